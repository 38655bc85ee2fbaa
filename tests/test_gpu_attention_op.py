"""Op-level tests of decode attention (-m gpu): one step through q3_attn_step — the one-launch kernel k_attn_fused (+ k_attn_merge /
k_attn_merge2), the three-launch path (k_qknorm_rope_kv + k_attn_decode + merge) and the code predictor's k_attn_cp — against
float64 numpy built from np_reference.rms_norm / rotate_half: per-head q/k RMSNorm, rotate-half RoPE at `pos`, append, GQA
head h -> kv head h // nrep, softmax(q.K^T * 128^-0.5).V. All three heads / kv-heads ratios (1, 2, 4) and the split counts that
take another merge (1 none, 2 k_attn_merge2, 3 / 16 the 16-wide merge, 17 / 64 the 64-wide one) run here.

Checked per case: `out` and the appended K row against f64, the appended V row bit-equal to the v part of qkv, and every other
element of both caches — filled with random data beyond `pos` too — bit-identical to what went in.

Tolerance. The same op in plain numpy float32 on these inputs deviates from f64 by at most D_REF (relative to max |out| of the
case; worst over every case of this file, measured on the CPU — _d_ref() below recomputes it). A kernel gets 4 * D_REF: a factor
of two for another summation order, another for a fast exp. The appended K row (a norm and a rotation, no sum over keys) gets the
same rule with its own D_REF_K."""
import functools

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from np_reference import rms_norm, rotate_half, rope_cos_sin

pytestmark = pytest.mark.gpu

EPS = 1e-6
HD = 128
RATIOS = [(2, 2), (2, 1), (4, 2), (4, 1)]          # heads / kv heads = 1, 2, 2, 4
SPLITS = [1, 2, 3, 16, 17, 64]
# fewer keys than splits (1, 2, 16 keys against 17 / 64 splits: empty splits must contribute nothing), key counts around a multiple
# of the chunk, the last slot of the cache
POS8 = (0, 1, 15, 16, 17, 63, 200, 255)
HOT = 5.3          # logit of an aligned key = 128^-0.5 * HOT * |q|^2 ~ 60 with |q|^2 ~ 128


@functools.lru_cache(maxsize=None)
def _rope(max_seq):
    c, s = rope_cos_sin(1.0e6, HD, np.arange(max_seq))
    return c.astype(np.float32), s.astype(np.float32)


def _norm_rope(x, w, pos, max_seq, dtype):
    """x [B][heads][128] -> per-head RMSNorm * w, rotate-half RoPE at pos[b]"""
    c, s = _rope(max_seq)
    c = c.astype(dtype)[pos][:, None, :]; s = s.astype(dtype)[pos][:, None, :]
    return rotate_half(rms_norm(x.astype(dtype), w.astype(dtype), dtype(EPS)), c, s)


@functools.lru_cache(maxsize=None)
def _case(nh, nkv, max_seq, pos, stress=False):
    """inputs of one step (read-only, shared by the variants and split counts that run it)"""
    B = len(pos); nrep = nh // nkv
    rng = np.random.default_rng(nh * 1000 + nkv * 100 + max_seq + sum(pos) * 7 + B + (5 if stress else 0))
    qkv = rng.standard_normal((B, (nh + 2 * nkv) * HD)).astype(np.float32)
    qw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kc = rng.standard_normal((B, nkv, max_seq, HD)).astype(np.float32)
    vc = rng.standard_normal((B, nkv, max_seq, HD)).astype(np.float32)
    p = np.array(pos, dtype=np.int32)
    if stress:
        # one key per row ~60 logits above the rest (for the first q head of every kv head): row 0 in the first split (position 0),
        # row 1 in the last cached position, row 2 the new position itself (k = q in front of a k-norm weight of HOT)
        assert B == 3 and min(pos) >= 2
        kw = (HOT * np.ones(HD)).astype(np.float32)
        qw = np.ones(HD, dtype=np.float32)
        qr = _norm_rope(qkv[:, :nh * HD].reshape(B, nh, HD), qw, p, max_seq, np.float64)
        for g in range(nkv):
            kc[0, g, 0] = (HOT * qr[0, g * nrep]).astype(np.float32)
            kc[1, g, pos[1] - 1] = (HOT * qr[1, g * nrep]).astype(np.float32)
            qkv[2, nh * HD + g * HD:nh * HD + (g + 1) * HD] = qkv[2, g * nrep * HD:(g * nrep + 1) * HD]
    for a in (qkv, qw, kw, kc, vc, p):
        a.setflags(write=False)
    return dict(nh=nh, nkv=nkv, max_seq=max_seq, pos=p, qkv=qkv, qw=qw, kw=kw, kc=kc, vc=vc)


def _reference(c, dtype=np.float64):
    """(out [B][nh*128], appended K rows [B][nkv][128]) in `dtype` arithmetic"""
    nh, nkv, pos = c["nh"], c["nkv"], c["pos"]
    B = len(pos); nrep = nh // nkv
    qkv = c["qkv"]
    qr = _norm_rope(qkv[:, :nh * HD].reshape(B, nh, HD), c["qw"], pos, c["max_seq"], dtype)
    kr = _norm_rope(qkv[:, nh * HD:(nh + nkv) * HD].reshape(B, nkv, HD), c["kw"], pos, c["max_seq"], dtype)
    v = qkv[:, (nh + nkv) * HD:].reshape(B, nkv, HD).astype(dtype)
    out = np.zeros((B, nh, HD), dtype=dtype)
    scale = dtype(HD ** -0.5)
    for b in range(B):
        L = int(pos[b]) + 1
        for h in range(nh):
            g = h // nrep
            K = np.concatenate([c["kc"][b, g, :L - 1].astype(dtype), kr[b, g][None]], 0)
            V = np.concatenate([c["vc"][b, g, :L - 1].astype(dtype), v[b, g][None]], 0)
            sc = (K @ qr[b, h]) * scale
            pr = np.exp(sc - sc.max()); pr = pr / pr.sum()
            out[b, h] = pr @ V
    return out.reshape(B, nh * HD), kr


@functools.lru_cache(maxsize=None)
def _ref64(key):
    return _reference(_case(*key))


def _all_case_keys():
    keys = []
    for (nh, nkv) in RATIOS:
        keys.append((nh, nkv, 256, POS8))
        keys.append((nh, nkv, 256, (37,)))
        keys.append((nh, nkv, 256, (37, 37, 37)))
        keys.append((nh, nkv, 256, (200, 200, 200), True))
        for p in (0, 1, 3, 4, 7, 8, 15):
            for B in (1, 8, 64):
                keys.append((nh, nkv, 17, (p,) * B))
    return keys


def _d_ref():
    """worst deviation of float32 numpy from float64 over every case of this file: (out, appended K row), relative to the case's max"""
    d = dk = 0.0
    for key in _all_case_keys():
        o64, k64 = _ref64(key)
        o32, k32 = _reference(_case(*key), np.float32)
        d = max(d, float(np.abs(o32 - o64).max() / np.abs(o64).max()))
        dk = max(dk, float(np.abs(k32 - k64).max() / np.abs(k64).max()))
    return d, dk


WORST = {}


def _run(variant, key, n_splits):
    c = _case(*key)
    o64, k64 = _ref64(key)
    nh, nkv, pos = c["nh"], c["nkv"], c["pos"]
    B = len(pos)
    rc, rs = _rope(c["max_seq"])
    out, kc, vc = q.attn_step(variant, c["qkv"], pos, c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], nh, nkv, n_splits)
    what = f"variant {variant} nh={nh} nkv={nkv} splits={n_splits} pos={[int(v) for v in pos[:8]]} B={B}"
    assert np.isfinite(out).all(), what
    dev = float(np.abs(out - o64).max() / np.abs(o64).max())
    bi = np.arange(B)
    k_new = kc[bi, :, pos]; v_new = vc[bi, :, pos]                      # [B][nkv][128]
    dev_k = float(np.abs(k_new - k64).max() / np.abs(k64).max())
    WORST[variant] = max(WORST.get(variant, 0.0), dev)
    print(f"{what}: out dev {dev:.3e} (bound {4 * D_REF:.3e}), K row dev {dev_k:.3e} (bound {4 * D_REF_K:.3e}); worst of variant so far {WORST[variant]:.3e}")
    assert dev <= 4 * D_REF, f"{what}: out deviates {dev:.3e} > {4 * D_REF:.3e}"
    assert dev_k <= 4 * D_REF_K, f"{what}: appended K row deviates {dev_k:.3e} > {4 * D_REF_K:.3e}"
    v_in = c["qkv"][:, (nh + nkv) * HD:].reshape(B, nkv, HD)
    assert (v_new.view(np.uint32) == v_in.view(np.uint32)).all(), f"{what}: appended V row is not the v part of qkv"
    # nothing but row `pos` of each (sequence, kv head) changed
    keep = np.ones(kc.shape[:3], dtype=bool); keep[bi, :, pos] = False
    assert (kc.view(np.uint32)[keep] == c["kc"].view(np.uint32)[keep]).all(), f"{what}: K cache written outside the appended row"
    assert (vc.view(np.uint32)[keep] == c["vc"].view(np.uint32)[keep]).all(), f"{what}: V cache written outside the appended row"


# measured with _d_ref() on the CPU (numpy float32 against float64, every case of this file): 3.98e-7 for `out` (the worst case is a
# softmax-stress one), 1.75e-7 for the appended K row. The GPU bounds are therefore 1.6e-6 and 7.0e-7.
D_REF = 3.98e-7
D_REF_K = 1.75e-7
assert 4 * D_REF <= 2e-5          # a looser figure would mean the inputs are ill-conditioned


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("n_splits", SPLITS)
@pytest.mark.parametrize("nh,nkv", RATIOS)
def test_eight_rows_mixed_positions(variant, nh, nkv, n_splits):
    _run(variant, (nh, nkv, 256, POS8), n_splits)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("nh,nkv", RATIOS)
def test_equal_positions(variant, nh, nkv):
    for B in (1, 3):
        for n_splits in (1, 2, 16, 17):
            _run(variant, (nh, nkv, 256, (37,) * B), n_splits)


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("nh,nkv", RATIOS)
def test_softmax_stress(variant, nh, nkv):
    """one key ~60 logits above the rest — in the first split, in the last cached position, and as the new position: every other
    split's own maximum is far below the global one and must merge to (next to) nothing, without NaN"""
    key = (nh, nkv, 256, (200, 200, 200), True)
    c = _case(*key)
    o64, _ = _ref64(key)
    # the inputs do what they claim: the hot key carries nearly all the weight of the first head of every kv head
    nrep = nh // nkv
    for g in range(nkv):
        h = g * nrep
        assert np.abs(o64[0, h * HD:(h + 1) * HD] - c["vc"][0, g, 0]).max() < 1e-6
        assert np.abs(o64[1, h * HD:(h + 1) * HD] - c["vc"][1, g, 199]).max() < 1e-6
        assert np.abs(o64[2, h * HD:(h + 1) * HD] - c["qkv"][2, (nh + nkv + g) * HD:(nh + nkv + g + 1) * HD]).max() < 1e-6
    for n_splits in SPLITS:
        _run(variant, key, n_splits)


@pytest.mark.parametrize("nh,nkv", RATIOS)
@pytest.mark.parametrize("B", [1, 8, 64])
def test_code_predictor_kernel(nh, nkv, B):
    for p in (0, 1, 3, 4, 7, 8, 15):  # k_attn_cp<4> (0 .. 3) / <8> (4 .. 7) / <16> (8 .. 15): the first and last position of each
        _run(2, (nh, nkv, 17, (p,) * B), 1)


def test_code_predictor_kernel_refuses_what_it_cannot_run():
    def refused(key, n_splits, status):
        c = _case(*key)
        rc, rs = _rope(c["max_seq"])
        with pytest.raises(_lib.Q3Error) as e:
            q.attn_step(2, c["qkv"], c["pos"], c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], c["nh"], c["nkv"], n_splits)
        assert e.value.status == status
    refused((4, 2, 17, (16,)), 1, 7)                   # position 16: beyond the kernel's 16 keys
    refused((4, 2, 17, (7,)), 2, 7)                    # more than one split
    refused((4, 2, 256, (37,)), 1, 7)                  # max_seq >= 256 does not fit the packed argument
    refused((4, 2, 17, (3, 4, 3)), 1, 1)               # one static position for every row
