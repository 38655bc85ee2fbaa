"""FP8 weights on the 4-row tiles (-m gpu; DESIGN 4.1a, "fp8-all"): k_gemv_w8r4 over the image k_w8_build4 makes, against float64
over the DEQUANTISED weights inside the family's bound and bit for bit on integer data, and an "fp8-all" model held to the CPU oracle."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import synth, _lib
import oracle as O
from common import rel_err, synthetic_prompt, top2_margin
from np_reference import rms_norm, silu
from test_gpu_linear_paths import TOL, EPS, SENT, CONFIGS, RESID, SILU, SWIGLU, _y_buf, _check_untouched
from test_gpu_parity import MARGIN_EPS
from test_gpu_w8 import PROJ, _cols, _run, _weights
from w8_cases import quantize

pytestmark = pytest.mark.gpu


# (N, K): one tile; N % 4 != 0 with a half-empty last tile and three scale blocks; K % 128 != 0; a talker projection
@pytest.mark.parametrize("N,K", [(8, 256), (38, 384), (64, 520), (1024, 2048)])
def test_kernel_against_float64(N, K):
    wb, _, _, w64 = _weights(N, K)
    i = 0
    for M in (1, 2, 3, 5, 8):              # one row group, partly and wholly filled; two
        for (epi, norm, bias) in CONFIGS:
            pad, zero_n = i % 5 == 0, (N * 4 + 4 if i % 7 == 1 else 0)
            what = f"w8r4 M={M} N={N} K={K} epi={epi} norm={norm} bias={bias} pad={pad}"
            rng = np.random.default_rng((M * 1000003 + N * 101 + K) * 8 + epi * 2 + int(norm))
            x = np.full((M, K + 4 if pad else K), 3.0e5, dtype=np.float32)       # beyond K: what a read past the row's end would drag in
            x[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
            kw = {}
            x64 = x[:, :K].astype(np.float64)
            if norm:
                kw["norm_w"] = (1.0 + 0.1 * rng.standard_normal(K)).astype(np.float32)
                x64 = rms_norm(x64, kw["norm_w"].astype(np.float64), EPS)
            ref = x64 @ w64.T
            if bias:
                kw["bias"] = rng.standard_normal(N).astype(np.float32)
                ref = ref + kw["bias"]
            if epi == RESID:
                kw["resid"] = np.full((M, N + 4 if pad else N), 9.0e5, dtype=np.float32)
                kw["resid"][:, :N] = rng.standard_normal((M, N)).astype(np.float32)
                ref = kw["resid"][:, :N].astype(np.float64) + ref
            elif epi == SILU:
                ref = silu(ref)
            elif epi == SWIGLU:
                kw["w2_bf16"], _, _, w264 = _weights(N, K, 1)
                ref = silu(ref) * (x64 @ w264.T)
            zb = np.full(zero_n + 64, SENT, dtype=np.float32) if zero_n else None
            kw.update(dict(zero_buf=zb, zero_n=zero_n) if zero_n else {})
            y =q.linear_ex(x, wb, eps=EPS, epi=epi, tiled=4, y=_y_buf(M, N, pad), **kw)
            err = rel_err(y[:M, :N], ref)
            print(f"{what}: rel_err {err:.3e}")
            assert err < TOL, f"{what}: rel_err {err:.3e}"
            _check_untouched(y, M, N, what)
            if zero_n:
                assert (zb[:zero_n].view(np.uint32) == 0).all() and (zb[zero_n:].view(np.uint32) == SENT.view(np.uint32)).all(), what
            i += 1


@pytest.mark.parametrize("M", [1, 8])
@pytest.mark.parametrize("N,K", [(38, 520), (64, 2048)])
def test_integer_data_bit_for_bit(M, N, K):
    """sixteen +-1 weights per row (exact in e4m3 at scale 1) times integers below 2^20, plus integers below 2^16: every partial sum
    is an integer below 2^24, so any order of f32 additions gives the integer result — a dropped mid / lo plane, a lane on the wrong
    k or scale block, or a read past K (3e5 there) does not"""
    rng = np.random.default_rng(N * 31 + K + M)
    w = np.zeros((N, K), dtype=np.float32)
    for n in range(N):
        cols = rng.choice(K - 1, 15, replace=False)
        w[n, cols] = rng.choice([-1.0, 1.0], 15); w[n, K - 1] = 1.0          # the row's last k always counts
    x = np.full((M, K + 4), 3.0e5, dtype=np.float32)
    x[:, :K] = rng.integers(-(2 ** 20) + 1, 2 ** 20, (M, K)).astype(np.float32)
    bias = rng.integers(-(2 ** 16) + 1, 2 ** 16, N).astype(np.float32)
    resid = rng.integers(-(2 ** 16) + 1, 2 ** 16, (M, N)).astype(np.float32)
    ref = x[:, :K].astype(np.int64) @ w.astype(np.int64).T
    assert np.abs(ref).max() + 2 ** 17 < 2 ** 24
    wb = synth.f32_to_bf16(w).reshape(N, K)
    y = q.linear_ex(x, wb, bias=bias, tiled=4)
    assert (y.astype(np.int64) == ref + bias.astype(np.int64)).all(), np.argwhere(y != ref + bias)[:4]
    y = q.linear_ex(x, wb, bias=bias, resid=resid, epi=RESID, tiled=4)
    assert (y.astype(np.int64) == ref + bias.astype(np.int64) + resid.astype(np.int64)).all()


@pytest.mark.parametrize("kw", [dict(M=9), dict(M=4, ksplit=2)])
def test_refused_launch_leaves_y_alone(kw):
    M = kw.pop("M")
    y = np.full((M, 64), SENT, dtype=np.float32)
    with pytest.raises(_lib.Q3Error) as e:
        q.linear_ex(np.ones((M, 512), dtype=np.float32), _weights(64, 512)[0], y=y, tiled=4, **kw)
    assert e.value.status == 7 and (y.view(np.uint32) == SENT.view(np.uint32)).all()


@pytest.fixture(scope="module")
def pair():
    """test_gpu_w8's tiny model and oracle over one checkpoint whose projections went through quantise -> dequantise"""
    cfg = q.tiny()
    cfg.hidden, cfg.inter, cfg.cp_hidden, cfg.cp_inter, cfg.name = 256, 256, 128, 256, "tiny_w8"
    om = O.OracleModel(cfg)
    gm = q.Qwen3TTS(cfg, 0)
    for name, arr, dt in synth.synthetic_checkpoint(cfg, gm._h, 11):
        if name.endswith(".weight") and any(p in name for p in PROJ) and not name.startswith("decoder."):
            arr = synth.f32_to_bf16(quantize(synth.bf16_to_f32(arr).reshape(-1, _cols(cfg, name)))[2].astype(np.float32)).reshape(-1)
        gm.set_tensor(name, arr, dt); om.set_tensor(name, arr, dt)
    gm.finalize(); om.finalize(3)
    yield cfg, gm, om
    gm.close()


@pytest.mark.parametrize("B", [1, 3])
def test_fp8_all_model_matches_oracle(pair, B, monkeypatch):
    cfg, gm, om = pair
    frames = 8
    utts = [q.Utterance(synthetic_prompt(11, i), seed=42 + i) for i in range(B)]
    before, _ = _run(gm, utts, frames)
    try:
        gm.set_weight_format("fp8")
        info8, bytes8 = gm.weight_info(), _run(gm, utts, frames)[1]
        gm.set_weight_format("fp8-all")
        info = gm.weight_info()
        assert gm.weight_format == "fp8-all" and info["fp8_bytes"] > info8["fp8_bytes"] and info["matrices"] >= info8["matrices"], (info, info8)
        codes, bytes_all = _run(gm, utts, frames)
        monkeypatch.setenv("Q3_AQL", "0")
        graph, _ = _run(gm, utts, frames)
        monkeypatch.delenv("Q3_AQL")
        assert bytes_all < bytes8, (bytes_all, bytes8)
        gm.set_weight_format("fp8")
        assert gm.weight_info() == info8 and _run(gm, utts, frames)[1] == bytes8
    finally:
        gm.set_weight_format("bf16")
    after, _ = _run(gm, utts, frames)
    for b in range(B):
        np.testing.assert_array_equal(codes[b], graph[b])                 # own queue (fence-free boundaries) == hipGraphLaunch
        np.testing.assert_array_equal(after[b], before[b])
        osess = O.OracleSession(om, utts[b], q.SynthesisOptions(max_length=frames, seed=42, eos_token_id=None))
        ocodes, otl, ocl = osess.generate(capture=True)
        osess.close()
        bad = np.argwhere(codes[b] != ocodes)
        if len(bad):          # tolerated only at an oracle near-tie (test_gpu_parity's allowance)
            f, g = bad[0]
            assert (top2_margin(otl[f]) if g == 0 else top2_margin(ocl[f][g - 1])) < MARGIN_EPS, (b, f, g)
