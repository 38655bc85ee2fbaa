"""Op-level tests of the long-prompt prefill kernels (-m gpu): q3_kernels_prefill.hip one launch at a time, against float64 numpy.
Inputs, shape tables (each row names the rule it is chosen against) and references live in prefill_ops_cases.py; what needs no GPU
— the D_REF recomputation, the integer-input bound, the table of picks, the reference against plain loops — is in
test_prefill_ops_reference.py.

GEMM (q3_gemm_ex -> launch_row_den / k_row_den, launch_split_rows / k_split_rows, ONE launch_lm_gemm: k_lm_gemm with the split in
the kernel or over planes, k_lm_gemm2, k_lm_gemm3 + k_gemm_splitk_reduce). Three checks per case, the rules of
test_gpu_linear_paths.py:
  * dense random inputs against f64 on the bf16-rounded weights, rel_err < 2e-5;
  * exact inputs (no norm, EPI_NONE / EPI_RESID): integer activations below 2^20, 16 weights of +-1 per row, integer bias / residual
    below 2^16 — every bf16x3 product and every partial sum in any order (range sums included) is an integer below 2^24, so y must
    equal the integer result bit for bit;
  * nothing else is written: sentinels survive in rows M..M_alloc and columns N..ldy. The planes buffer (whole 128-row tiles) and the
    split-K workspace are NaN-filled by the entry, so a stored row past M, an unzeroed K..Kpad or an unwritten range shows.
Bit-identity (the file's own promises, array_equal): k_split 1 / 2 / 4 / 8 of geometry 3; a row alone (M = 1) against the same row in
an M = 130 launch, at index 0 and at index 129; geometry 1 over planes against geometry 1 with the split in the kernel — both
kernels run one MFMA loop (stage, k-step, lo / mid / hi plane) on the same split of x * norm_w, only the staging differs.

Prefill attention (q3_attn_prefill_ex -> k_qknorm_rope_kv, k_kv_planes for the bf16x3 kernel, ONE launch_attn_prefill:
k_attn_prefill, k_attn_prefill_mfma, k_attn_prefill_t, k_attn_prefill_x3, then k_attn_merge2 — the two-halves merge). Checked per
case: `out` and the appended K rows against f64, the appended V rows bit-equal to the v part of qkv, every other cache element
bit-identical to what went in, `out` beyond nh * 128 columns untouched. Tolerance: the rule of test_gpu_attention_op.py — the same
reference in numpy float32 deviates from f64 by at most D_REF over this file's cases; a kernel gets 4 * D_REF (a factor of two for
another summation order, another for a fast exp), the appended K row 4 * D_REF_K. The softmax-stress cases lie beyond the others'
figure in numpy float32 already (1.74e-6 against 1.61e-6), so they are held to 4 * D_REF_STRESS, their own by the same rule.

Measured on an MI355X (worst over every case of this file):
  GEMM rel_err:      geometry 1 in-kernel split 4.2e-7, geometry 1 over planes 4.2e-7 (the same bits), geometry 2 7.4e-7,
                     geometry 3 6.0e-7 (bound 2e-5)
  attention dev / D_REF:  VALU 0.44, gen2 MFMA 1.50, transposed f32 MFMA 1.52, bf16x3 1.21 (bound 4); appended K rows 0.80 of
                     D_REF_K (bound 4)
The bf16x3 kernel's dropped product terms (at most 3 * 2^-24 |a||b| each) are of f32's own size, and it shows: it sits next to
the float32 reference's own deviation and below the two f32-MFMA generations, well inside the bound.

Unaligned base. k_attn_prefill_t / k_attn_prefill_x3 over two key halves used to return NaN for a chunk whose base is not a
multiple of 32 (smallest case: base_pos = 100, rps = 100, heads 2 / 2): the second half starts at tile h0, a wave whose 32 positions
straddle that tile's start has queries that see the tile fully masked, and exp(-inf - -inf) poisoned their record. The kernels now
take 0 as the reference of a lane whose running max is still -inf (every aligned case keeps its bits: there the max is finite from
the first tile on); test_unaligned_base holds them to the f64 bound for one and two halves."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from common import rel_err
import prefill_ops_cases as C
from prefill_ops_cases import NONE, RESID, SILU, SWIGLU, G1_SPLIT, G1_PLANES, G2, G3, VALU, GEN2, GEN_T, X3, HD, EPS, SENT
from prefill_ops_cases import D_REF, D_REF_K, D_REF_STRESS

pytestmark = pytest.mark.gpu

# the shapes below are chosen against the DEFAULT dispatch; these knobs would silently move a case to another kernel
KNOBS = ["Q3_GEMM_GEO1", "Q3_GEMM_GEO", "Q3_GEMM_NSPLIT", "Q3_GEMM3_SUP", "Q3_GEMM3_KSPLIT", "Q3_GEMM_NO_PLANES", "Q3_PREFILL_ROWS"]
assert [k for k in os.environ if k in KNOBS or k.startswith("Q3_PREFILL_ATTN_")] == [], \
    "prefill knobs set: the shape tables would not reach the kernels they name"

TOL = 2e-5
WORST_GEMM = {}
WORST_ATTN = {}
UNSUPPORTED = 7


def _same_bits(a, b):
    return (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).all()


def _check_untouched(y, M, N, what):
    assert _same_bits(y[M:], np.full_like(y[M:], SENT)), f"{what}: rows beyond M written"
    assert _same_bits(y[:, N:], np.full_like(y[:, N:], SENT)), f"{what}: columns beyond N written"


# ---------------------------------------------------------------- GEMM
def _dense(geometry, M, N, K, epi, norm, bias, pad, k_split=0, sup=(0, 0), want=None):
    """one launch on dense random inputs against f64; returns (y [M][N], path)"""
    what = f"geometry {geometry} M={M} N={N} K={K} epi={epi} norm={norm} bias={bias} k_split={k_split} sup={sup} pad={pad}"
    x, wb, kw, ref = C.dense_case(M, N, K, epi, norm, bias, pad)
    y, path = q.gemm_ex(x, wb, eps=EPS, epi=epi, geometry=geometry, k_split=k_split, sup=sup, y=C.y_buf(M, N, pad), **kw)
    assert path[0] == (geometry if want is None else want), f"{what}: ran geometry {path[0]}"
    if k_split:
        assert path[2] == k_split, f"{what}: ran k_split {path[2]}"
    err = rel_err(y[:M, :N], ref)
    WORST_GEMM[path[0]] = max(WORST_GEMM.get(path[0], 0.0), err)
    print(f"{what} path={path}: rel_err {err:.3e}; worst of geometry so far {WORST_GEMM[path[0]]:.3e}")
    assert np.isfinite(y[:M, :N]).all(), f"{what}: non-finite output (an unwritten plane, workspace range or record)"
    assert err < TOL, f"{what}: rel_err {err:.3e}"
    _check_untouched(y, M, N, what)
    return y[:M, :N], path


def _exact(geometry, M, N, K, epi, bias, pad, k_split=0):
    what = f"exact geometry {geometry} M={M} N={N} K={K} epi={epi} bias={bias} k_split={k_split} pad={pad}"
    x, wb, kw, ref, _ = C.exact_case(M, N, K, epi, bias, pad)
    assert np.abs(ref).max() < (1 << 24)
    ref32 = ref.astype(np.float32)
    y, path = q.gemm_ex(x, wb, epi=epi, geometry=geometry, k_split=k_split, y=C.y_buf(M, N, pad), **kw)
    assert path[0] == geometry
    bad = np.argwhere(y[:M, :N].view(np.uint32) != ref32.view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} of {M * N} outputs differ from the integer result, first at {bad[0]}: " \
                          f"{y[tuple(bad[0])]!r} != {ref32[tuple(bad[0])]!r}"
    _check_untouched(y, M, N, what)


def _shape_rows(geometry):
    return [r for r in C.GEMM_SHAPES if r[0] == geometry]


def _run_row(row):
    geometry, N, K, Ms, k_splits = row
    i = 0
    for M in Ms:
        for (epi, norm, bias) in C.GEMM_CONFIGS:
            n = C.gemm_n(geometry, N, epi)
            pad = i % 4 == 0
            ys = {}
            for ks in k_splits:
                ys[ks], path = _dense(geometry, M, n, K, epi, norm, bias, pad, k_split=ks)
                if not norm and epi in (NONE, RESID):
                    _exact(geometry, M, n, K, epi, bias, pad, k_split=ks)
            # "an output is the same sum in the same order" whatever k_split is — the engine's own included
            for ks in k_splits[1:]:
                assert _same_bits(ys[ks], ys[k_splits[0]]), f"geometry {geometry} M={M} N={n} K={K} epi={epi}: k_split {ks} and {k_splits[0]} differ in bits"
            i += 1


@pytest.mark.parametrize("row", _shape_rows(G1_SPLIT), ids=lambda r: f"N{r[1]}-K{r[2]}")
def test_gemm_geometry1_split_in_kernel(row):
    _run_row(row)


@pytest.mark.parametrize("row", _shape_rows(G1_PLANES), ids=lambda r: f"N{r[1]}-K{r[2]}")
def test_gemm_geometry1_planes(row):
    _run_row(row)


@pytest.mark.parametrize("row", _shape_rows(G2), ids=lambda r: f"N{r[1]}-K{r[2]}")
def test_gemm_geometry2(row):
    _run_row(row)


@pytest.mark.parametrize("row", _shape_rows(G3), ids=lambda r: f"N{r[1]}-K{r[2]}")
def test_gemm_geometry3(row):
    _run_row(row)


def test_gemm_engine_picks():
    """what the engine's own pick runs, read back through `path` (geometry, k_ranges, k_split, n_split)"""
    _, path = _dense(-1, 130, 384, 128, NONE, False, True, False, want=G2)          # N % 256 != 0: geometry 2, three N tiles in one unit
    assert path == (G2, 1, 1, 1)
    _, path = _dense(G2, 130, 256, 128, NONE, False, True, False)                   # forced (the engine takes geometry 3): two units
    assert path == (G2, 1, 1, 2)
    _, path = _dense(G2, 130, 128, 128, NONE, False, True, False)
    assert path == (G2, 1, 1, 1)
    _, path = _dense(-1, 130, 256, 1024, NONE, False, True, False, want=G3)         # 2 tiles on 256 CUs: the ranges are spread
    assert path[1] == 8 and path[2] > 1, path
    _, path = _dense(-1, 130, 256, 384, NONE, False, True, False, want=G3)          # six stages: one range, nothing to spread
    assert path == (G3, 1, 1, 1)
    _, path = _dense(-1, 130, 64, 40, NONE, False, True, False, want=G1_PLANES)     # N % 128 != 0: geometry 1 over planes
    assert path == (G1_PLANES, 1, 1, 1)
    for (geometry, N, K, Ms, _) in C.GEMM_SHAPES:                                    # the host-only table agrees with what ran
        if geometry != G1_SPLIT:
            assert q.gemm_path(Ms[1], N, K)[0] == q.gemm_ex(C.dense_case(Ms[1], N, K, NONE, False, False, False)[0], C.weights(N, K, 0)[0])[1][0]


@pytest.mark.parametrize("sup", C.SUPER_TILE["sups"], ids=lambda s: f"sup{s[0]}x{s[1]}")
def test_gemm_geometry3_super_tile_walk(sup):
    """6 x 9 tiles (6 x 18 for SwiGLU) under super-tiles whose edges divide neither: every output written exactly once"""
    M, N, K = C.SUPER_TILE["M"], C.SUPER_TILE["N"], C.SUPER_TILE["K"]
    for (epi, norm, bias) in ((NONE, False, True), (RESID, False, False), (SWIGLU, True, False)):
        _dense(G3, M, N, K, epi, norm, bias, True, sup=sup)
    _exact(G3, M, N, K, NONE, True, True)


@pytest.mark.parametrize("geometry,N,K", [(G1_SPLIT, 192, 72), (G1_PLANES, 192, 72), (G2, 256, 320), (G3, 256, 384), (G3, 256, 1024)])
def test_gemm_row_bits_do_not_depend_on_the_batch(geometry, N, K):
    """"a position prefilled by this GEMM gets the same bits whatever batch it is prefilled in": row m of an M = 130 launch equals the
    M = 1 launch of that row alone, and the same row placed at index 129 instead of 0 (geometry 3 at K = 1024: under whatever
    k_split the engine picks for each M)"""
    M = 130
    for (epi, norm, bias) in ((NONE, True, False), (SILU, False, True), (RESID, False, True), (SWIGLU, True, False)):
        n = C.gemm_n(geometry, N, epi)
        x, wb, kw, _ = C.dense_case(M, n, K, epi, norm, bias, False)
        y, _ = q.gemm_ex(x, wb, eps=EPS, epi=epi, geometry=geometry, **kw)
        for m in (0, 64, 129):
            kw1 = dict(kw)
            if "resid" in kw1:
                kw1["resid"] = kw["resid"][m:m + 1]
            y1, _ = q.gemm_ex(x[m:m + 1], wb, eps=EPS, epi=epi, geometry=geometry, **kw1)
            assert _same_bits(y1[0], y[m]), f"geometry {geometry} N={n} K={K} epi={epi}: row {m} alone differs from row {m} of M=130"
        xs = x.copy(); xs[[0, 129]] = xs[[129, 0]]
        kws = dict(kw)
        if "resid" in kws:
            kws["resid"] = kw["resid"].copy(); kws["resid"][[0, 129]] = kws["resid"][[129, 0]]
        ys, _ = q.gemm_ex(xs, wb, eps=EPS, epi=epi, geometry=geometry, **kws)
        assert _same_bits(ys[129], y[0]) and _same_bits(ys[0], y[129]), f"geometry {geometry} N={n} K={K} epi={epi}: a row's bits depend on its index"


@pytest.mark.parametrize("N,K", [(64, 72), (192, 128)])
def test_gemm_geometry1_planes_equal_split_in_kernel(N, K):
    """k_lm_gemm<PL> stages what k_split_rows wrote, k_lm_gemm<!PL> splits the same x * norm_w itself; the MFMA loop is one piece
    of code (stage, k-step, lo / mid / hi), so the two must agree in every bit"""
    for M in (1, 130):
        for (epi, norm, bias) in C.GEMM_CONFIGS:
            n = N
            x, wb, kw, _ = C.dense_case(M, n, K, epi, norm, bias, True)
            ya, _ = q.gemm_ex(x, wb, eps=EPS, epi=epi, geometry=G1_SPLIT, **kw)
            yb, _ = q.gemm_ex(x, wb, eps=EPS, epi=epi, geometry=G1_PLANES, **kw)
            assert _same_bits(ya, yb), f"M={M} N={n} K={K} epi={epi} norm={norm}: planes and in-kernel split differ in bits"


def _refused(fn):
    with pytest.raises(_lib.Q3Error) as e:
        fn()
    assert e.value.status == UNSUPPORTED, e.value


@pytest.mark.parametrize("geometry,N,K", [(G1_SPLIT, 64, 72), (G1_PLANES, 64, 72), (G2, 128, 72), (G3, 256, 128), (-1, 256, 1024)])
def test_gemm_refuses_what_it_cannot_run(geometry, N, K):
    """a norm in front of EPI_RESID / EPI_SILU, SwiGLU without a norm or without a second matrix: Q3_UNSUPPORTED, y untouched"""
    M = 5
    rng = np.random.default_rng(N + K)
    x = rng.standard_normal((M, K)).astype(np.float32)
    for (epi, norm, w2) in C.GEMM_REFUSED:
        kw = {}
        if norm:
            kw["norm_w"] = np.ones(K, dtype=np.float32)
        if w2:
            kw["w2_bf16"] = C.weights(N, K, 1)[0]
        if epi == RESID:
            kw["resid"] = np.zeros((M, N), dtype=np.float32)
        y = C.y_buf(M, N, True)
        _refused(lambda: q.gemm_ex(x, C.weights(N, K, 0)[0], epi=epi, geometry=geometry, y=y, **kw))
        assert _same_bits(y, np.full_like(y, SENT)), f"geometry {geometry} epi={epi} norm={norm}: y written by a refused launch"


def test_gemm_refuses_a_pick_the_shape_does_not_allow():
    x = np.ones((5, 72), dtype=np.float32)
    for (geometry, N, K, extra) in [(G2, 64, 72, {}),                    # N % 128
                                    (G3, 256, 72, {}),                   # Kpad % 128
                                    (G3, 128, 128, {}),                  # N % 256
                                    (G3, 256, 128, dict(k_split=2)),     # one range: nothing to split
                                    (G3, 256, 1024, dict(k_split=3)),    # not a divisor of the 8 ranges
                                    (G1_PLANES, 64, 36, {})]:            # planes need K % 8
        y = C.y_buf(5, N, False)
        xx = np.ones((5, K), dtype=np.float32)
        _refused(lambda: q.gemm_ex(xx, C.weights(N, K, 0)[0], geometry=geometry, y=y, **extra))
        assert _same_bits(y, np.full_like(y, SENT))


# ---------------------------------------------------------------- prefill attention
def _attn(key, kernel, halves, use_planes=False, d_ref=None):
    """one launch against f64; returns (out [rows][nh*128], path)"""
    c = C.attn_case(*key)
    o64, k64 = C.attn_ref64(key)
    nh, nkv, rps, base, n_seq = c["nh"], c["nkv"], c["rps"], c["base"], c["n_seq"]
    rows = n_seq * rps
    d_ref = D_REF if d_ref is None else d_ref
    rc, rs = C.rope(c["max_seq"])
    out_in = np.full((rows, nh * HD + 4), SENT, dtype=np.float32)
    out, kc, vc, path = q.attn_prefill_ex(c["qkv"], n_seq, base, c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], nh, nkv, kernel=kernel,
                                          halves=halves, use_planes=use_planes, out=out_in)
    what = f"kernel {kernel} halves={halves} nh={nh} nkv={nkv} rps={rps} base={base} n_seq={n_seq} path={path}"
    assert path[1] == halves and (kernel < 0 or path[0] == kernel), what
    assert _same_bits(out[:, nh * HD:], np.full((rows, 4), SENT)), f"{what}: out written beyond nh * 128 columns"
    out = out[:, :nh * HD]
    assert np.isfinite(out).all(), f"{what}: {int((~np.isfinite(out)).sum())} non-finite outputs"
    dev = float(np.abs(out - o64).max() / np.abs(o64).max())
    k_new = kc[:, :, base:base + rps].transpose(0, 2, 1, 3).reshape(rows, nkv, HD)
    v_new = vc[:, :, base:base + rps].transpose(0, 2, 1, 3).reshape(rows, nkv, HD)
    dev_k = float(np.abs(k_new - k64).max() / np.abs(k64).max())
    WORST_ATTN[path[0]] = max(WORST_ATTN.get(path[0], 0.0), dev / d_ref)
    WORST_ATTN["K"] = max(WORST_ATTN.get("K", 0.0), dev_k / D_REF_K)
    print(f"{what}: out dev {dev:.3e} = {dev / d_ref:.2f} D_REF (bound 4), K row dev {dev_k:.3e} = {dev_k / D_REF_K:.2f} D_REF_K; "
          f"worst dev / D_REF so far {WORST_ATTN}")
    assert dev <= 4 * d_ref, f"{what}: out deviates {dev:.3e} > {4 * d_ref:.3e}"
    assert dev_k <= 4 * D_REF_K, f"{what}: appended K rows deviate {dev_k:.3e} > {4 * D_REF_K:.3e}"
    v_in = c["qkv"][:, (nh + nkv) * HD:].reshape(rows, nkv, HD)
    assert _same_bits(v_new, v_in), f"{what}: appended V rows are not the v part of qkv"
    keep = np.ones(kc.shape[:3], dtype=bool); keep[:, :, base:base + rps] = False
    assert (kc.view(np.uint32)[keep] == c["kc"].view(np.uint32)[keep]).all(), f"{what}: K cache written outside the appended rows"
    assert (vc.view(np.uint32)[keep] == c["vc"].view(np.uint32)[keep]).all(), f"{what}: V cache written outside the appended rows"
    return out, path


@pytest.mark.parametrize("nh,nkv", C.RATIOS)
@pytest.mark.parametrize("kernel", [VALU, GEN2, GEN_T, X3])
def test_attn_against_f64(kernel, nh, nkv):
    nrep = nh // nkv
    pairs = [p for p in C.attn_kernels(nrep) if p[0] == kernel]
    if not pairs:          # the VALU kernel takes ratios 1 and 2 only: anything else is refused, nothing written
        c = C.attn_case(nh, nkv, 33, 0, 5)
        rc, rs = C.rope()
        out = np.full((5 * 33, nh * HD), SENT, dtype=np.float32)
        _refused(lambda: q.attn_prefill_ex(c["qkv"], 5, 0, c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], nh, nkv, kernel=VALU, out=out))
        assert _same_bits(out, np.full_like(out, SENT))
        return
    for (_, halves) in pairs:
        for row in C.attn_rows(kernel, nrep):
            _attn((nh, nkv) + row, kernel, halves)


@pytest.mark.parametrize("nh,nkv", C.RATIOS)
def test_attn_softmax_stress(nh, nkv):
    """one key ~60 logits above the rest for the last row of each sequence — at position 0 (first tile, first key half), at the last
    key of the tile in front of the row's own tile, at the row's own position: the online-softmax rescale across tiles and across
    the two halves, where every other tile's own maximum is far below the global one"""
    key = C.attn_stress_key(nh, nkv)
    c = C.attn_case(*key)
    o64, _ = C.attn_ref64(key)
    nrep = nh // nkv; rps, base = c["rps"], c["base"]
    tile0 = (base + rps - 1) // 32 * 32
    for g in range(nkv):          # the inputs do what they claim: the hot key carries nearly all the weight
        h = g * nrep
        assert np.abs(o64[rps - 1, h * HD:(h + 1) * HD] - c["vc"][0, g, 0]).max() < 1e-6
        assert np.abs(o64[2 * rps - 1, h * HD:(h + 1) * HD] - c["vc"][1, g, tile0 - 1]).max() < 1e-6
        assert np.abs(o64[3 * rps - 1, h * HD:(h + 1) * HD] - c["qkv"][3 * rps - 1, (nh + nkv + g) * HD:(nh + nkv + g + 1) * HD]).max() < 1e-6
    for (kernel, halves) in C.attn_kernels(nrep):
        _attn(key, kernel, halves, d_ref=D_REF_STRESS)


@pytest.mark.parametrize("nh,nkv", [(2, 2), (2, 1)])
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("kernel", [GEN_T, X3])
def test_attn_cached_prefix_and_batch_bits(kernel, halves, nh, nkv):
    """what prefill_gemm and prefix_usable_pages_of rest on: positions from a cached prefix boundary (one query block) on see the
    arithmetic of the uncached run, and a sequence's rows do not depend on the other sequences of the launch"""
    nrep = nh // nkv
    qb = C.query_block(kernel, nrep)
    R, P0 = 2 * qb + 40, qb
    max_seq = 640                                     # 2 * 256 + 40 rows of the bf16x3 kernel at ratio 1
    c = C.attn_case(nh, nkv, R, 0, 1, False, max_seq)
    rc, rs = C.rope(max_seq)
    run = lambda qkv, n_seq, base, kc, vc: q.attn_prefill_ex(qkv, n_seq, base, c["qw"], c["kw"], EPS, rc, rs, kc, vc, nh, nkv, kernel=kernel, halves=halves)
    out0, kc0, vc0, _ = run(c["qkv"], 1, 0, c["kc"], c["vc"])
    assert np.isfinite(out0).all()
    # the same prompt from P0 on, over a cache that holds the first run's K/V of [0, P0) (and other data behind it)
    kc1 = c["kc"].copy(); vc1 = c["vc"].copy()
    kc1[:, :, :P0] = kc0[:, :, :P0]; vc1[:, :, :P0] = vc0[:, :, :P0]
    out1, kc1o, vc1o, _ = run(c["qkv"][P0:], 1, P0, kc1, vc1)
    assert _same_bits(out1, out0[P0:]), f"kernel {kernel} halves {halves} nh={nh} nkv={nkv}: rows from the cached prefix boundary {P0} on differ in bits"
    assert _same_bits(kc1o[:, :, :R], kc0[:, :, :R]) and _same_bits(vc1o[:, :, :R], vc0[:, :, :R])
    # five sequences in one launch (10 or 5 pairs over the 8 XCD slots) against each alone
    c5 = C.attn_case(nh, nkv, 33, 128, 5, False, max_seq)
    out5, _, _, _ = run(c5["qkv"], 5, 128, c5["kc"], c5["vc"])
    for s in (0, 3, 4):
        o1, _, _, _ = run(c5["qkv"][s * 33:(s + 1) * 33], 1, 128, c5["kc"][s:s + 1], c5["vc"][s:s + 1])
        assert _same_bits(o1, out5[s * 33:(s + 1) * 33]), f"kernel {kernel} halves {halves}: sequence {s} of 5 differs from its own launch"


@pytest.mark.parametrize("halves", [1, 2])
def test_attn_engine_pick_is_the_kernel_it_names(halves):
    """kernel -1: the engine's pick without / with K/V planes is the transposed f32 kernel / the bf16x3 kernel, bit for bit"""
    key = (4, 2, 200, 128, 1)
    for (use_planes, named) in ((False, GEN_T), (True, X3)):
        out_e, path = _attn(key, -1, halves, use_planes=use_planes)
        assert path == (named, halves) == q.attn_prefill_path(4, 2, use_planes, halves)
        out_f, _ = _attn(key, named, halves)
        assert _same_bits(out_e, out_f)


def test_attn_refuses_key_halves_of_the_first_generations():
    c = C.attn_case(2, 1, 33, 0, 5)
    rc, rs = C.rope()
    for kernel in (VALU, GEN2):
        out = np.full((5 * 33, 2 * HD), SENT, dtype=np.float32)
        _refused(lambda: q.attn_prefill_ex(c["qkv"], 5, 0, c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], 2, 1, kernel=kernel, halves=2, out=out))
        assert _same_bits(out, np.full_like(out, SENT))


@pytest.mark.parametrize("nh,nkv", C.RATIOS)
@pytest.mark.parametrize("halves", [1, 2])
@pytest.mark.parametrize("kernel", [GEN_T, X3])
def test_attn_unaligned_base(kernel, halves, nh, nkv):
    """a chunk whose base is not a multiple of 32 (a wave's positions straddle a tile start; the engine never does this, the
    launcher accepts it): finite and inside the f64 bound, for one key half and for two"""
    for base in C.UNALIGNED_BASES:
        _attn((nh, nkv, 100, base, 1), kernel, halves)
