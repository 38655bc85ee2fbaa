"""Op-level tests of the bf16-weight GEMV family (-m gpu): every kernel `launch_linear` can pick under the default dispatch,
driven one launch at a time through q3_linear_ex and compared with float64 numpy.

Three checks per case:
  * dense random inputs: RMSNorm / bias / residual / SiLU / SwiGLU in f64 on the bf16-rounded weights and the f32 inputs,
    rel_err < 2e-5 (the figure of test_linear_matches_oracle);
  * exact inputs (no norm, EPI_NONE / EPI_RESID): integer activations below 2^20, 16 weights of +-1 per row, integer bias and
    residual below 2^16 — every bf16x3 product and every f32 partial sum in ANY order is an integer below 2^24, so y must equal
    the integer result bit for bit. A dropped or misplaced mid / lo plane, a wrong lane-to-k mapping or a read past K changes it;
  * nothing else is written: y comes back with its sentinel in rows M..M_alloc and columns N..ldy, and the clearing side job
    (LinArgs::zero) zeroes [0, zero_n) and not one float more.

The shape table names, per row, the rule of launch_gemv_t / launch_gemv_sk2 / launch_gemv4_t / launch_gemv_tiled /
gemm_wide_impl it is chosen against (tiles = ceil(N / 16), S = up32(K) / 32; 4-row tiles: S4 = up128(K) / 128)."""
import functools
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import synth, _lib
import oracle as O
from common import rel_err
from np_reference import rms_norm, silu

pytestmark = pytest.mark.gpu

# the shapes below are chosen against the DEFAULT dispatch; these knobs are read once per process and would silently move a
# case to another kernel
KNOBS = ["Q3_GEMV_WAVES", "Q3_GEMV_NO_LDS", "Q3_GEMV_BIG8", "Q3_GEMV_NO_GU24", "Q3_GEMV_NO_HALF", "Q3_WIDE_NO_GEMM", "Q3_WIDE2",
         "Q3_WIDE2_NT2", "Q3_WIDE_WG_CAP", "Q3_WIDE_MIN_CHUNKS", "Q3_WIDE_GEMM_MIN"]
assert [k for k in KNOBS if k in os.environ] == [], "dispatch knobs set: the shape table would not reach the kernels it names"

NONE, RESID, SILU, SWIGLU = 0, 1, 2, 3
TOL = 2e-5
EPS = 1e-6
SENT = np.float32(-7.0625e33)            # sentinel around y / behind the zeroed range: no kernel computes this value
# (epilogue, fused norm, bias): everything the launchers accept — a norm in front of EPI_RESID / EPI_SILU is refused
CONFIGS = [(NONE, False, True), (NONE, True, False), (RESID, False, True), (SILU, False, False), (SWIGLU, True, False), (SWIGLU, False, True)]
SK2_CONFIGS = [(NONE, False, False), (NONE, False, True), (RESID, False, False), (RESID, False, True)]


@functools.lru_cache(maxsize=4)
def _weights(N, K, which):
    """bf16 bits [N][K] and their f64 values, shared by every case of a shape (read-only)."""
    rng = np.random.default_rng(N * 7919 + K * 31 + which)
    bits = synth.f32_to_bf16((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).reshape(N, K)
    w64 = synth.bf16_to_f32(bits).reshape(N, K).astype(np.float64)
    bits.setflags(write=False); w64.setflags(write=False)
    return bits, w64


def _y_buf(M, N, pad):
    y = np.full((M + (2 if pad else 1), N + (4 if pad else 0)), SENT, dtype=np.float32)
    return y


def _check_untouched(y, M, N, what):
    assert (y[M:].view(np.uint32) == SENT.view(np.uint32)).all(), f"{what}: rows beyond M written"
    assert (y[:, N:].view(np.uint32) == SENT.view(np.uint32)).all(), f"{what}: columns beyond N written"


def _dense(M, N, K, epi, norm, bias, tiled, ksplit=1, use_ws=True, pad=False, oracle=False, zero_n=0):
    """one launch on dense random inputs against f64; returns the GPU result [M][N]"""
    what = f"M={M} N={N} K={K} epi={epi} norm={norm} bias={bias} tiled={tiled} ksplit={ksplit} ws={use_ws} pad={pad}"
    rng = np.random.default_rng((M * 1000003 + N * 101 + K) * 8 + epi * 2 + int(norm))
    ldx = K + 4 if pad else K
    x = np.full((M, ldx), 3.0e5, dtype=np.float32)          # beyond K: values a read past the row's end would drag into the sum
    x[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
    wb, w64 = _weights(N, K, 0)
    kw = {}
    x64 = x[:, :K].astype(np.float64)
    if norm:
        nw = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
        kw["norm_w"] = nw
        x64 = rms_norm(x64, nw.astype(np.float64), EPS)
    ref = x64 @ w64.T
    if bias:
        b = rng.standard_normal(N).astype(np.float32)
        kw["bias"] = b
        ref = ref + b
    if epi == RESID:
        r = np.full((M, N + 4 if pad else N), 9.0e5, dtype=np.float32)
        r[:, :N] = rng.standard_normal((M, N)).astype(np.float32)
        kw["resid"] = r
        ref = r[:, :N].astype(np.float64) + ref
    elif epi == SILU:
        ref = silu(ref)
    elif epi == SWIGLU:
        wb2, w264 = _weights(N, K, 1)
        kw["w2_bf16"] = wb2
        ref = silu(ref) * (x64 @ w264.T)
    zb = None
    if zero_n:
        zb = np.full(zero_n + 64, SENT, dtype=np.float32)
        kw["zero_buf"] = zb; kw["zero_n"] = zero_n
    y = q.linear_ex(x, wb, eps=EPS, epi=epi, tiled=tiled, ksplit=ksplit, use_ws=use_ws, y=_y_buf(M, N, pad), **kw)
    err = rel_err(y[:M, :N], ref)
    print(f"{what}: rel_err {err:.3e}")
    assert err < TOL, f"{what}: rel_err {err:.3e}"
    _check_untouched(y, M, N, what)
    if zero_n:
        assert (zb[:zero_n].view(np.uint32) == 0).all(), f"{what}: side job left part of [0, {zero_n}) uncleared"
        assert (zb[zero_n:].view(np.uint32) == SENT.view(np.uint32)).all(), f"{what}: side job wrote beyond zero_n"
    if oracle:          # EPI_NONE without a norm: the CPU oracle's linear inside the same bound, as in test_linear_matches_oracle
        assert epi == NONE and not norm
        yo = np.zeros((M, N), dtype=np.float32)
        wf = np.ascontiguousarray(w64.astype(np.float32))
        bo = kw.get("bias")
        O.olib.q3o_linear(O.ptr(np.ascontiguousarray(x[:, :K])), O.ptr(wf), O.ptr(bo) if bo is not None else None, O.ptr(yo), M, N, K)
        assert rel_err(yo, ref) < TOL and rel_err(y[:M, :N], yo) < TOL, what
    return y[:M, :N]


@functools.lru_cache(maxsize=4)
def _exact_weights(N, K):
    """[N][K] with exactly 16 entries of +-1 per row, placed so that over the rows every 32-wide k-step and the K tail carry one"""
    rng = np.random.default_rng(N * 131 + K)
    steps = (K + 31) // 32
    assert N * 16 >= steps
    w = np.zeros((N, K), dtype=np.float32)
    if steps >= 16:          # 16 consecutive steps (mod steps) per row are distinct: one entry in each
        st = (np.arange(N)[:, None] * 16 + np.arange(16)[None, :]) % steps
        width = np.minimum(32, K - st * 32)
        off = np.minimum((rng.random((N, 16)) * width).astype(np.int64), width - 1)
        w[np.arange(N)[:, None], st * 32 + off] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(N, 16))
    else:
        for n in range(N):
            st = (n * 16 + np.arange(16)) % steps
            for s in np.unique(st):
                cnt = int((st == s).sum()); width = min(32, K - s * 32)
                off = rng.choice(width, size=cnt, replace=False)
                w[n, s * 32 + off] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=cnt)
    # the test's own inputs: 16 nonzeros per row, every k-step (the tail step included) hit by some row
    assert ((w != 0).sum(axis=1) == 16).all()
    hit = (w != 0).any(axis=0)
    assert all(hit[s * 32:min(K, s * 32 + 32)].any() for s in range(steps))
    bits = synth.f32_to_bf16(w).reshape(N, K)
    assert (synth.bf16_to_f32(bits).reshape(N, K) == w).all()
    bits.setflags(write=False); w.setflags(write=False)
    return bits, w.astype(np.int64)


XMAX = (1 << 20) - (1 << 14)        # 16 * XMAX + 2 * 2^16 < 2^24: every partial sum, bias and residual included, is exact in f32


def _exact(M, N, K, epi, tiled, ksplit=1, use_ws=True, pad=False, bias=True):
    what = f"exact M={M} N={N} K={K} epi={epi} tiled={tiled} ksplit={ksplit} ws={use_ws} pad={pad}"
    rng = np.random.default_rng(M * 7 + N * 3 + K + epi)
    ldx = K + 4 if pad else K
    xi = rng.integers(-XMAX, XMAX + 1, size=(M, K))
    x = np.full((M, ldx), 3.0e5, dtype=np.float32); x[:, :K] = xi
    wb, wi = _exact_weights(N, K)
    ref = xi @ wi.T
    kw = {}
    if bias:
        bi = rng.integers(-(1 << 16) + 1, 1 << 16, size=N)
        kw["bias"] = bi.astype(np.float32); ref = ref + bi
    if epi == RESID:
        ri = rng.integers(-(1 << 16) + 1, 1 << 16, size=(M, N))
        r = np.full((M, N + 4 if pad else N), 9.0e5, dtype=np.float32); r[:, :N] = ri
        kw["resid"] = r; ref = ref + ri
    assert np.abs(ref).max() < (1 << 24)
    ref32 = ref.astype(np.float32)
    runs = 2 if ksplit == 2 else 1          # split-K: the two halves meet through atomics — the same bits every time
    for _ in range(runs):
        y = q.linear_ex(x, wb, epi=epi, tiled=tiled, ksplit=ksplit, use_ws=use_ws, y=_y_buf(M, N, pad), **kw)
        bad = np.argwhere(y[:M, :N].view(np.uint32) != ref32.view(np.uint32))
        assert len(bad) == 0, f"{what}: {len(bad)} of {M * N} outputs differ from the integer result, first at {bad[0]}: " \
                              f"{y[tuple(bad[0])]!r} != {ref32[tuple(bad[0])]!r}"
        _check_untouched(y, M, N, what)


def _family(shapes, Ms, configs, tiled, pad_every=5, zero_at=None, **kw):
    """dense + exact checks over shapes x Ms x configs; one case in `pad_every` runs with ldx = K + 4, ldy = N + 4 (at least one per call)"""
    i = 0
    for (N, K) in shapes:
        for M in Ms:
            for (epi, norm, bias) in configs:
                pad = i % pad_every == 0
                zn = zero_at if (zero_at and i == 1) else 0
                _dense(M, N, K, epi, norm, bias, tiled, pad=pad, oracle=(epi == NONE and not norm), zero_n=zn, **kw)
                if not norm and epi in (NONE, RESID):
                    _exact(M, N, K, epi, tiled, pad=pad, bias=bias, **kw)
                i += 1


# ---------------------------------------------------------------- 16-row tiles, M <= 16
# k_gemv_mfma<8 waves>: neither LDS pick ((tiles < 256 and 32 < S <= 64) or (M > 8 and S >= 96)) nor S >= 96 nor the 4-wave SwiGLU
# rule (S == 64): N=48 K=64 -> tiles 3, S 2; N=40 K=136 -> ragged third tile, Kpad 160, S 5, K tail of 8; N=4096 K=1024 -> tiles 256,
# S 32 (the largest S of this family at a full chip of tiles). M <= 2: CO = false; M <= 8: HALF; M > 8: full 16-column tiles.
@pytest.mark.parametrize("N,K", [(48, 64), (40, 136), (4096, 1024)])
def test_tile16_eight_waves(N, K):
    _family([(N, K)], [1, 2, 3, 5, 8, 9, 13, 16], CONFIGS, 1, zero_at=N * 3 + 4)       # zero_n / tiles is not whole: 148 / 3, 124 / 3, 12292 / 256


# k_gemv_lds: tiles < 256 and 32 < S <= 64 -> N=64 K=1056 (tiles 4, S 33), N=40 K=2048 (tiles 3, S 64) at every M;
# M > 8 and S >= 96 -> N=32 K=3072 (S 96) and K=3080 (Kpad 3104, S 97, tail of 8) at M = 9, 16
@pytest.mark.parametrize("N,K,Ms", [(64, 1056, [1, 2, 3, 8, 9, 16]), (40, 2048, [1, 2, 3, 8, 9, 16]), (32, 3072, [9, 16]), (32, 3080, [9, 16])])
def test_tile16_lds_staged(N, K, Ms):
    _family([(N, K)], Ms, CONFIGS, 1, zero_at=N * 2 + 4)


# k_gemv_mfma<16 waves, HALF>: S >= 96 and M <= 8 (beyond 8 rows the LDS-staged kernel takes these shapes, so the 16-wave
# instance without HALF is not reachable under the default dispatch): S = 96, 97 (ragged wave slices + K tail), 192
@pytest.mark.parametrize("K", [3072, 3080, 6144])
def test_tile16_sixteen_waves(K):
    _family([(32, K)], [1, 2, 3, 5, 8], CONFIGS, 1, zero_at=36)


# k_gemv_mfma<4 waves> (SwiGLU only): S == 64 and tiles >= 256 and not the 24-row kernel — N=4096 K=2048 (tiles 256, 256 % 3 != 0)
# with and without a norm; N=5376 (tiles 336: inside the 24-row window) WITH a bias, which that kernel does not take
@pytest.mark.parametrize("N,norm,bias", [(4096, True, False), (4096, False, False), (4096, False, True), (5376, True, True)])
def test_tile16_four_wave_swiglu(N, norm, bias):
    for i, M in enumerate([1, 2, 3, 8, 9, 16]):           # M <= 2: CO = false, M <= 8: HALF, else full tiles
        _dense(M, N, 2048, SWIGLU, norm, bias, 1, pad=(i == 0), zero_n=(N + 4 if i == 1 else 0))


# k_gemv_gu24: SwiGLU + norm, no bias, tiles % 3 == 0, 224 <= tiles / 3 * 2 <= 288, S >= 64, S % 8 == 0, K == Kpad —
# N=5376 (224 workgroups) and N=6912 (288), the two ends of the window, K=2048. M <= 2 / <= 8 / > 8: one instance each
@pytest.mark.parametrize("N", [5376, 6912])
def test_tile16_gu24(N):
    for i, M in enumerate([1, 2, 3, 8, 9, 16]):
        _dense(M, N, 2048, SWIGLU, True, False, 1, pad=(i == 0), zero_n=(N + 4 if i == 1 else 0))


# ---------------------------------------------------------------- split-K in two (k_gemv_sk2)
# ksplit = 2 needs S >= 16: K=512 (S 16: groups of 4), K=1056 (S 33, odd: the halves are 16 and 17 steps), K=3072 / 6144 (S / 2 a
# multiple of 48: groups of 6). M <= 8: HALF; M <= 16: full tile; M > 16: the row-block form (grid plane per 16 rows, ragged last).
@pytest.mark.parametrize("N", [40, 1024])
@pytest.mark.parametrize("K", [512, 1056, 3072, 6144])
def test_split_k(N, K):
    i = 0
    for M in [1, 3, 8, 9, 16, 17, 33, 64]:
        for (epi, _, bias) in SK2_CONFIGS:
            pad = i % 5 == 0
            _dense(M, N, K, epi, False, bias, 1, ksplit=2, pad=pad, oracle=(epi == NONE), zero_n=(M * N + 4 if i % 7 == 1 else 0))
            _exact(M, N, K, epi, 1, ksplit=2, pad=pad, bias=bias)
            i += 1


# ---------------------------------------------------------------- 4-row tiles (k_gemv_mfma4), M <= 16
# waves by S4: K=64 -> 1; 256 -> 2; 384 -> S4 3 over 2 waves (ragged); 512 -> 4; 1024 -> 8; 3072 -> 8 waves x 3 steps: the
# group-of-3 instances (no norm, not SwiGLU); 136 -> Kpad 256 with a K tail. N=6: ragged second tile. M -> MG 1 (<= 4), 2 (<= 8), 4.
@pytest.mark.parametrize("N", [6, 1024])
@pytest.mark.parametrize("K", [64, 256, 384, 512, 1024, 3072, 136])
def test_tile4(N, K):
    _family([(N, K)], [1, 4, 5, 8, 9, 16], CONFIGS, 2, zero_at=N * 2 + 4)


# ---------------------------------------------------------------- wide batches, 17 <= M <= 64
# k_gemv_wide (no workspace): MT = ceil(M / 16) = 2 / 3 / 4 with full and ragged last column tiles; N=520: ragged last weight tile
@pytest.mark.parametrize("N", [520, 2048])
@pytest.mark.parametrize("K", [136, 2048])
def test_wide_gemv(N, K):
    _family([(N, K)], [17, 32, 33, 48, 49, 64], CONFIGS, 1, use_ws=False, zero_at=N * 17 + 4)


# k_wide_gemm + k_wide_epilogue (workspace, N % 128 == 0, K % 128 == 0): 64 weight rows per workgroup at N=128 K=256 (one
# 128-row group cannot fill the chip), 128 rows at N=2048 K=3072 (192 workgroups); K=384: three 128-column chunks. SwiGLU with a
# norm belongs to k_wide2_* (below); without one it takes the generic two-matrix epilogue.
WIDE_GEMM_CONFIGS = [(NONE, False, True), (NONE, True, False), (RESID, False, True), (SILU, False, False), (SWIGLU, False, False)]


@pytest.mark.parametrize("N", [128, 1024, 2048])
@pytest.mark.parametrize("K", [256, 384, 2048, 3072])
def test_wide_gemm(N, K):
    _family([(N, K)], [17, 33, 64], WIDE_GEMM_CONFIGS, 1, use_ws=True, zero_at=N * 17 + 4)


def test_wide_gemm_falls_back_outside_its_shapes():
    """N=520 with a workspace: gemm_wide_impl answers hipErrorNotSupported and the dispatcher itself takes k_gemv_wide"""
    _family([(520, 2048), (520, 136)], [17, 64], CONFIGS, 1, use_ws=True)


# k_wide2_split + k_wide2_swiglu: SwiGLU + norm, no bias, K % 256 == 0; N=1024: one tile per workgroup, N=4224 (> 4096): two;
# M -> MT 2 / 3 / 4. With a bias, or K=384 (not a multiple of 256), the same launch takes the generic split path.
@pytest.mark.parametrize("N", [1024, 4224])
@pytest.mark.parametrize("K", [256, 2048])
def test_wide2_swiglu(N, K):
    for i, M in enumerate([17, 33, 49, 64]):
        _dense(M, N, K, SWIGLU, True, False, 1, use_ws=True, pad=(i == 0), zero_n=(N * 3 + 4 if i == 1 else 0))
        _dense(M, N, K, SWIGLU, True, True, 1, use_ws=True, pad=(i == 1))
    for M in [17, 49]:
        _dense(M, N, 384, SWIGLU, True, False, 1, use_ws=True)


# ---------------------------------------------------------------- first-generation VALU kernel (row-major weights, M <= 8)
# N=40: one row per wave; N=4096: two rows per wave (N / 8 >= 512); K=136: a chunk that is no multiple of the wave's 512-float stride
@pytest.mark.parametrize("M,N,K", [(1, 40, 64), (3, 520, 136), (8, 4096, 1024)])
def test_rowmajor(M, N, K):
    _family([(N, K)], [M], CONFIGS, 0)


def test_engine_choice_matches_forced_tiling():
    """tiled = -1 is pick_mode: 4-row tiles for M <= 2 (or N <= 1024 up to 8 rows) unless K <= 1024 with N >= 2048"""
    for (M, N, K, mode) in [(2, 1024, 512, 2), (8, 1024, 512, 2), (9, 1024, 512, 1), (2, 2048, 1024, 1), (2, 2048, 2048, 2), (17, 1024, 512, 1)]:
        a = _dense(M, N, K, NONE, False, True, -1)
        b = _dense(M, N, K, NONE, False, True, mode)
        assert (a.view(np.uint32) == b.view(np.uint32)).all(), (M, N, K, mode)


# ---------------------------------------------------------------- refusals
def _refused(**kw):
    M, N, K = kw.pop("M", 4), kw.pop("N", 64), kw.pop("K", 512)
    rng = np.random.default_rng(1)
    x = rng.standard_normal((M, K)).astype(np.float32)
    w = synth.f32_to_bf16(rng.standard_normal((N, K)).astype(np.float32)).reshape(N, K)
    y = np.full((M, N), SENT, dtype=np.float32)
    if kw.pop("norm", False):
        kw["norm_w"] = np.ones(K, dtype=np.float32)
    if kw.get("epi") == RESID:
        kw["resid"] = np.ones((M, N), dtype=np.float32)
    with pytest.raises(_lib.Q3Error) as e:
        q.linear_ex(x, w, y=y, **kw)
    assert e.value.status in (1, 7) and len(str(e.value)) > 0
    assert (y.view(np.uint32) == SENT.view(np.uint32)).all()         # a refused launch leaves y alone


@pytest.mark.parametrize("tiled", [0, 1, 2])
def test_refusals(tiled):
    _refused(tiled=tiled, epi=RESID, norm=True)
    _refused(tiled=tiled, epi=SILU, norm=True)
    _refused(tiled=tiled, ksplit=3)
    _refused(tiled=tiled, K=12)                                     # K % 8 != 0
    if tiled == 1:
        _refused(tiled=1, M=20, epi=RESID, norm=True, use_ws=False)
        _refused(tiled=1, M=20, epi=SILU, norm=True, use_ws=True, N=128)
        _refused(tiled=1, M=20, ksplit=3)
        # split-K: no fused norm, no SiLU, at least 16 k-steps
        _refused(tiled=1, ksplit=2, norm=True)
        _refused(tiled=1, ksplit=2, epi=SILU)
        _refused(tiled=1, ksplit=2, K=256)
        _refused(tiled=1, ksplit=2, K=256, M=20)
    else:
        _refused(tiled=tiled, ksplit=2)
