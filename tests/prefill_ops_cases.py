"""Inputs, shape tables and float64 references shared by tests/test_gpu_prefill_ops.py and tests/test_gpu_prefill_paged.py (the
kernels, -m gpu) and tests/test_prefill_ops_reference.py (what can be checked without a GPU). TEST INFRASTRUCTURE — no test lives here.

GEMM: y = epilogue(rms_norm(x, w) @ W^T) on bf16-rounded weights, as in tests/test_gpu_linear_paths.py.
Attention: one prefill chunk — n_seq sequences of rps rows at positions base_pos .. base_pos + rps - 1 over a contiguous cache:
per-head q/k RMSNorm, rotate-half RoPE at base_pos + r, row r attends the cache positions [0, base_pos) as given plus the chunk's
own rows 0..r (GQA: head h -> kv head h // nrep), softmax(q.K^T * 128^-0.5).V."""
import functools

import numpy as np

from qwen3_tts_rs_amd import synth
from np_reference import rms_norm, rotate_half, rope_cos_sin, silu

NONE, RESID, SILU, SWIGLU = 0, 1, 2, 3
EPS = 1e-6
HD = 128
MAX_SEQ = 512
PAGE = 128                               # positions of a K/V page
SLAB_SLOTS = 32                          # pages of a slab
SENT = np.float32(-7.0625e33)            # sentinel around y / in `out`: no kernel computes this value
# geometry codes of q3_gemm_ex / q3_gemm_path
G1_SPLIT, G1_PLANES, G2, G3 = 0, 1, 2, 3
# kernel codes of q3_attn_prefill_ex / q3_attn_prefill_path
VALU, GEN2, GEN_T, X3 = 0, 1, 2, 3

# (epilogue, fused norm, bias): everything launch_lm_gemm accepts
GEMM_CONFIGS = [(epi, norm, bias) for (epi, norm) in ((NONE, False), (NONE, True), (RESID, False), (SILU, False), (SWIGLU, True)) for bias in (True, False)]
# ... and everything it refuses: (epilogue, fused norm, second matrix)
GEMM_REFUSED = [(RESID, True, False), (SILU, True, False), (SWIGLU, False, True), (SWIGLU, True, False)]


# ---------------------------------------------------------------- GEMM inputs
@functools.lru_cache(maxsize=8)
def weights(N, K, which):
    """bf16 bits [N][K] and their f64 values, shared by every case of a shape (read-only)."""
    rng = np.random.default_rng(N * 7919 + K * 31 + which)
    bits = synth.f32_to_bf16((rng.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32)).reshape(N, K)
    w64 = synth.bf16_to_f32(bits).reshape(N, K).astype(np.float64)
    bits.setflags(write=False); w64.setflags(write=False)
    return bits, w64


def y_buf(M, N, pad):
    return np.full((M + (2 if pad else 1), N + (4 if pad else 0)), SENT, dtype=np.float32)


def dense_case(M, N, K, epi, norm, bias, pad, seed=0):
    """(x [M][ldx], keyword arguments of q.gemm_ex, f64 reference [M][N]) on dense random inputs. pad: ldx = K + 4 with 3e5 beyond K
    (what a read past the row's end would drag into the sum), ldr = N + 4."""
    rng = np.random.default_rng((M * 1000003 + N * 101 + K) * 8 + epi * 2 + int(norm) + seed * 977)
    ldx = K + 4 if pad else K
    x = np.full((M, ldx), 3.0e5, dtype=np.float32)
    x[:, :K] = rng.standard_normal((M, K)).astype(np.float32)
    wb, w64 = weights(N, K, 0)
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
        wb2, w264 = weights(N, K, 1)
        kw["w2_bf16"] = wb2
        ref = silu(ref) * (x64 @ w264.T)
    return x, wb, kw, ref


XMAX = (1 << 20) - (1 << 14)        # 16 * XMAX + 2 * 2^16 < 2^24: every partial sum, bias and residual included, is exact in f32


@functools.lru_cache(maxsize=8)
def exact_weights(N, K):
    """bf16 bits and integer values [N][K] with exactly 16 entries of +-1 per row; over the rows every 32-wide k-step (the K tail
    included) carries one, so no k-step of any plane can be dropped unnoticed"""
    rng = np.random.default_rng(N * 131 + K)
    steps = (K + 31) // 32
    assert N >= steps and K >= 16
    w = np.zeros((N, K), dtype=np.float32)
    for n in range(N):          # one entry in k-step n % steps (so the rows cover every step), fifteen anywhere else
        s = n % steps
        first = s * 32 + int(rng.integers(min(32, K - s * 32)))
        rest = rng.choice(np.delete(np.arange(K), first), size=15, replace=False)
        cols = np.concatenate([[first], rest])
        w[n, cols] = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=16)
    assert ((w != 0).sum(axis=1) == 16).all()
    hit = (w != 0).any(axis=0)
    assert all(hit[s * 32:min(K, s * 32 + 32)].any() for s in range(steps))
    bits = synth.f32_to_bf16(w).reshape(N, K)
    assert (synth.bf16_to_f32(bits).reshape(N, K) == w).all()
    bits.setflags(write=False)
    return bits, w.astype(np.int64)


def exact_case(M, N, K, epi, bias, pad):
    """(x, bf16 weights, keyword arguments, integer reference [M][N], integer parts (xi, wi, bias, resid)) of the exact check"""
    assert epi in (NONE, RESID)
    rng = np.random.default_rng(M * 7 + N * 3 + K + epi)
    ldx = K + 4 if pad else K
    xi = rng.integers(-XMAX, XMAX + 1, size=(M, K))
    x = np.full((M, ldx), 3.0e5, dtype=np.float32); x[:, :K] = xi
    wb, wi = exact_weights(N, K)
    ref = xi @ wi.T
    kw = {}
    bi = ri = None
    if bias:
        bi = rng.integers(-(1 << 16) + 1, 1 << 16, size=N)
        kw["bias"] = bi.astype(np.float32); ref = ref + bi
    if epi == RESID:
        ri = rng.integers(-(1 << 16) + 1, 1 << 16, size=(M, N))
        r = np.full((M, N + 4 if pad else N), 9.0e5, dtype=np.float32); r[:, :N] = ri
        kw["resid"] = r; ref = ref + ri
    return x, wb, kw, ref, (xi, wi, bi, ri)


# ---------------------------------------------------------------- GEMM shape tables
# Each row: (geometry, N, K, Ms, k_splits) and the rule of launch_lm_gemm / the kernel it is chosen against. Kpad = up32(K); a
# stage is 64 k, so Kpad % 64 == 32 ends in a half stage. M = 1: one row of one tile; 127 / 130 / 257: a ragged last 128-row tile
# behind 0 / 1 / 2 whole ones. Every row runs every configuration of GEMM_CONFIGS: the ones with a norm go through k_row_den (one
# wave per row, 4 rows per workgroup: M = 1 / 127 / 130 / 257 leave 1 / 3 / 2 / 1 live waves in the last one) and k_split_rows<RMS>,
# the others through k_split_rows<false>. SwiGLU halves the workgroup's N tile in geometries 2 and 3 (gemm_n below), so there it
# runs at N = 64 / 128 / 192 and 128 / 256: the same tile counts as the other epilogues at twice the N.
GEMM_SHAPES = [
    # k_lm_gemm<.., PL = false> (the split in the kernel; K % 4 only): N = 64 one workgroup column, 192 three;
    # K = 36 -> Kpad 64 with a K tail inside a float4 group of zeros, K = 72 -> Kpad 96: the half stage, K = 128 two whole stages
    (G1_SPLIT, 64, 36, (1, 127, 130), (0,)), (G1_SPLIT, 192, 36, (1, 127, 130), (0,)),
    (G1_SPLIT, 64, 72, (1, 127, 130), (0,)), (G1_SPLIT, 192, 72, (1, 127, 130), (0,)),
    (G1_SPLIT, 64, 128, (1, 127, 130), (0,)), (G1_SPLIT, 192, 128, (1, 127, 130), (0,)),
    # k_lm_gemm<.., PL = true> over k_split_rows planes (K % 8): K = 40 -> Kpad 64, planes zeroed over 40..64
    (G1_PLANES, 64, 40, (1, 127, 130), (0,)), (G1_PLANES, 192, 40, (1, 127, 130), (0,)),
    (G1_PLANES, 64, 72, (1, 127, 130), (0,)), (G1_PLANES, 192, 72, (1, 127, 130), (0,)),
    (G1_PLANES, 64, 128, (1, 127, 130), (0,)), (G1_PLANES, 192, 128, (1, 127, 130), (0,)),
    # k_lm_gemm2: N = 128 one N tile (n_split 1), N = 256 two (n_split 2; forced: the engine takes geometry 3 there when Kpad % 128
    # == 0), N = 384 three (n_split falls back to 1; N % 256 != 0, so the engine's own pick: see test_gemm_engine_picks);
    # K = 72 -> the half stage, 128, 320 -> five stages (Kpad % 128 != 0). M = 257: three M tiles x n_split units = 6 < 8 XCD slots
    # (padding workgroups), M = 130 two
    (G2, 128, 72, (1, 130, 257), (0,)), (G2, 256, 72, (1, 130, 257), (0,)), (G2, 384, 72, (1, 130, 257), (0,)),
    (G2, 128, 128, (1, 130, 257), (0,)), (G2, 256, 128, (1, 130, 257), (0,)), (G2, 384, 128, (1, 130, 257), (0,)),
    (G2, 128, 320, (1, 130, 257), (0,)), (G2, 256, 320, (1, 130, 257), (0,)), (G2, 384, 320, (1, 130, 257), (0,)),
    # k_lm_gemm3 (Kpad % 128 == 0, N % 256 == 0): K = 128 -> k_ranges 1, two stages (one double-buffer round), K = 384 -> six
    # stages, one range; K = 1024 -> 16 stages, k_ranges 8 of spr = 2 stages; K = 2048 -> spr = 4. With 8 ranges every k_split
    # (k_gemm_splitk_reduce for 2 / 4 / 8) and the engine's own; N = 512 the engine's and 4
    (G3, 256, 128, (1, 130, 257), (0,)), (G3, 512, 128, (1, 130, 257), (0,)),
    (G3, 256, 384, (1, 130, 257), (0,)), (G3, 512, 384, (1, 130, 257), (0,)),
    (G3, 256, 1024, (1, 130, 257), (0, 1, 2, 4, 8)), (G3, 512, 1024, (1, 130, 257), (0, 4)),
    (G3, 256, 2048, (1, 130, 257), (0, 1, 2, 4, 8)), (G3, 512, 2048, (1, 130, 257), (0, 4)),
]
# the super-tile walk of k_lm_gemm3: 6 M tiles x 9 N tiles (18 for SwiGLU), neither a multiple of any super-tile edge below
SUPER_TILE = dict(M=647, N=2304, K=128, sups=((0, 0), (4, 8), (1, 8), (2, 3)))


def gemm_n(geometry, N, epi):
    """the N at which SwiGLU walks the same tiles as the other epilogues at N: geometries 2 and 3 halve the workgroup's N tile for
    the gate / up pair (64 / 128 instead of 128 / 256), geometry 1 keeps its 64 rows of each"""
    return N // 2 if epi == SWIGLU and geometry in (G2, G3) else N


# ---------------------------------------------------------------- attention inputs
@functools.lru_cache(maxsize=None)
def rope(max_seq=MAX_SEQ):
    c, s = rope_cos_sin(1.0e6, HD, np.arange(max_seq))
    return c.astype(np.float32), s.astype(np.float32)


def norm_rope(x, w, pos, dtype, max_seq=MAX_SEQ):
    """x [rows][heads][128] -> per-head RMSNorm * w, rotate-half RoPE at pos[row]"""
    c, s = rope(max_seq)
    c = c.astype(dtype)[pos][:, None, :]; s = s.astype(dtype)[pos][:, None, :]
    return rotate_half(rms_norm(x.astype(dtype), w.astype(dtype), dtype(EPS)), c, s)


HOT = 5.3          # logit of an aligned key = 128^-0.5 * HOT * |q|^2 ~ 60 with |q|^2 ~ 128
STRESS = dict(rps=20, base=128, n_seq=3)       # last row at position 147: tiles 0..4, its own tile starts at 128


@functools.lru_cache(maxsize=None)
def attn_case(nh, nkv, rps, base, n_seq, stress=False, max_seq=MAX_SEQ, shared=0):
    """inputs of one prefill chunk (read-only, shared by the kernels and halves counts that run it). shared: sequences 0 and 1 hold
    the same K/V in their first `shared` pages of 128 positions (a cached prefix they have in common)"""
    nrep = nh // nkv; rows = n_seq * rps
    rng = np.random.default_rng(nh * 1000 + nkv * 100 + rps * 13 + base * 7 + n_seq + (5 if stress else 0))
    qkv = rng.standard_normal((rows, (nh + 2 * nkv) * HD)).astype(np.float32)
    qw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kc = rng.standard_normal((n_seq, nkv, max_seq, HD)).astype(np.float32)      # random beyond base + rps too
    vc = rng.standard_normal((n_seq, nkv, max_seq, HD)).astype(np.float32)
    pos = (base + np.arange(rows) % rps).astype(np.int64)
    if stress:
        # for the LAST row of each sequence (first q head of every kv head) one key ~60 logits above the rest: sequence 0 at position 0
        # (the first tile, the first key half), sequence 1 at the last key of the 32-key tile in front of the row's own tile,
        # sequence 2 at the row's own position (k = q in front of a k-norm weight of HOT)
        assert n_seq == 3 and base >= 32 and (base + rps - 1) // 32 * 32 - 1 < base
        kw = (HOT * np.ones(HD)).astype(np.float32)
        qw = np.ones(HD, dtype=np.float32)
        qr = norm_rope(qkv[:, :nh * HD].reshape(rows, nh, HD), qw, pos, np.float64, max_seq)
        last = [s * rps + rps - 1 for s in range(3)]
        tile0 = (base + rps - 1) // 32 * 32
        for g in range(nkv):
            kc[0, g, 0] = (HOT * qr[last[0], g * nrep]).astype(np.float32)
            kc[1, g, tile0 - 1] = (HOT * qr[last[1], g * nrep]).astype(np.float32)
            qkv[last[2], nh * HD + g * HD:nh * HD + (g + 1) * HD] = qkv[last[2], g * nrep * HD:(g * nrep + 1) * HD]
    if shared:
        assert n_seq >= 2 and shared * PAGE <= base and not stress
        kc[1, :, :shared * PAGE] = kc[0, :, :shared * PAGE]; vc[1, :, :shared * PAGE] = vc[0, :, :shared * PAGE]
    for a in (qkv, qw, kw, kc, vc, pos):
        a.setflags(write=False)
    return dict(nh=nh, nkv=nkv, rps=rps, base=base, n_seq=n_seq, max_seq=max_seq, pos=pos, qkv=qkv, qw=qw, kw=kw, kc=kc, vc=vc)


def attn_reference(c, dtype=np.float64):
    """(out [rows][nh*128], appended K rows [rows][nkv][128]) in `dtype` arithmetic"""
    nh, nkv, rps, base, n_seq = c["nh"], c["nkv"], c["rps"], c["base"], c["n_seq"]
    rows = n_seq * rps; nrep = nh // nkv
    qkv = c["qkv"]
    qr = norm_rope(qkv[:, :nh * HD].reshape(rows, nh, HD), c["qw"], c["pos"], dtype, c["max_seq"])
    kr = norm_rope(qkv[:, nh * HD:(nh + nkv) * HD].reshape(rows, nkv, HD), c["kw"], c["pos"], dtype, c["max_seq"])
    v = qkv[:, (nh + nkv) * HD:].reshape(rows, nkv, HD).astype(dtype)
    out = np.zeros((rows, nh, HD), dtype=dtype)
    scale = dtype(HD ** -0.5)
    visible = np.arange(base + rps)[None, :] <= (base + np.arange(rps))[:, None]          # [row][key]: key position <= query position
    for s in range(n_seq):
        sl = slice(s * rps, (s + 1) * rps)
        for h in range(nh):
            g = h // nrep
            K = np.concatenate([c["kc"][s, g, :base].astype(dtype), kr[sl, g]], 0)
            V = np.concatenate([c["vc"][s, g, :base].astype(dtype), v[sl, g]], 0)
            sc = (qr[sl, h] @ K.T) * scale
            sc = np.where(visible, sc, dtype(-np.inf))
            pr = np.exp(sc - sc.max(axis=1, keepdims=True)); pr = pr / pr.sum(axis=1, keepdims=True)
            out[sl, h] = pr @ V
    return out.reshape(rows, nh * HD), kr


def attn_reference_naive(c):
    """the same op as plain loops over (row, head, key) in f64 — only to check attn_reference itself on a tiny case"""
    nh, nkv, rps, base, n_seq = c["nh"], c["nkv"], c["rps"], c["base"], c["n_seq"]
    rows = n_seq * rps; nrep = nh // nkv
    cs, sn = rope(c["max_seq"])
    qkv = c["qkv"].astype(np.float64)

    def nr(vec, w, p):
        y = vec / np.sqrt(np.mean(vec * vec) + EPS) * w.astype(np.float64)
        o = np.empty(HD)
        for i in range(64):
            co, si = float(cs[p, i]), float(sn[p, i])
            o[i] = y[i] * co - y[i + 64] * si
            o[i + 64] = y[i + 64] * co + y[i] * si
        return o
    out = np.zeros((rows, nh * HD)); kr = np.zeros((rows, nkv, HD))
    for r in range(rows):
        for g in range(nkv):
            kr[r, g] = nr(qkv[r, (nh + g) * HD:(nh + g + 1) * HD], c["kw"], base + r % rps)
    for r in range(rows):
        s, i = divmod(r, rps)
        for h in range(nh):
            g = h // nrep
            qv = nr(qkv[r, h * HD:(h + 1) * HD], c["qw"], base + i)
            logits = []; vals = []
            for p in range(base + i + 1):
                kk = c["kc"][s, g, p].astype(np.float64) if p < base else kr[s * rps + p - base, g]
                vv = c["vc"][s, g, p].astype(np.float64) if p < base else qkv[s * rps + p - base, (nh + nkv + g) * HD:(nh + nkv + g + 1) * HD]
                logits.append(float(np.dot(qv, kk)) / np.sqrt(128.0)); vals.append(vv)
            mx = max(logits)
            wts = [np.exp(l - mx) for l in logits]
            tot = sum(wts)
            out[r, h * HD:(h + 1) * HD] = sum(w_ * v_ for w_, v_ in zip(wts, vals)) / tot
    return out, kr


@functools.lru_cache(maxsize=None)
def attn_ref64(key):
    return attn_reference(attn_case(*key))


RATIOS = [(2, 2), (2, 1), (4, 2), (4, 1)]          # heads / kv heads = 1, 2, 2, 4


def query_block(kernel, nrep):
    """query rows per workgroup"""
    return 8 if kernel == VALU else (256 if kernel == X3 else 128) // nrep


def attn_kernels(nrep):
    """(kernel, halves) pairs that run at a heads / kv heads ratio: the VALU kernel takes 1 and 2 only, the first two generations
    have no key halves"""
    ks = [(GEN2, 1), (GEN_T, 1), (GEN_T, 2), (X3, 1), (X3, 2)]
    return ([(VALU, 1)] if nrep <= 2 else []) + ks


def attn_rows(kernel, nrep):
    """(rps, base_pos, n_seq) per kernel, each against one rule of the kernels (keys come in tiles of 32; a wave owns 32 query rows;
    tiles = (base + rps - 1) // 32 + 1 per workgroup of the last block; two halves cut at (tiles + 1) // 2)"""
    qb = query_block(kernel, nrep)
    return [
        (1, 0, 1),            # one row, one key: a single tile — with two halves the second is empty and its record must merge as nothing
        (31, 256, 3),         # less than a wave of rows behind 8 whole cached tiles; tiles = 9 (odd: halves of 5 and 4)
        (33, 0, 5),           # one row into a second wave / tile, no cache; 5 sequences x 2 kv heads = 10 pairs: a second XCD round, 6 padding slots
        (qb + 1, 128, 1),     # one row into a second query block (its workgroup has one live row), cached prefix of 4 tiles
        (200, 128, 1),        # several blocks, ragged last one; last position 327 -> 11 tiles (odd), causal edge inside every own tile
    ]


def attn_case_keys():
    """every (nh, nkv, rps, base, n_seq, stress) the GPU file runs through the f64 comparison — what D_REF is the worst case of"""
    keys = []
    for (nh, nkv) in RATIOS:
        nrep = nh // nkv
        for (kernel, _) in attn_kernels(nrep):
            for row in attn_rows(kernel, nrep):
                k = (nh, nkv) + row
                if k not in keys:
                    keys.append(k)
        for base in UNALIGNED_BASES:
            keys.append((nh, nkv, 100, base, 1))
    return keys


UNALIGNED_BASES = (100, 130)


def attn_stress_key(nh, nkv):
    return (nh, nkv, STRESS["rps"], STRESS["base"], STRESS["n_seq"], True)


def d_ref(keys):
    """worst deviation of float32 numpy from float64 over `keys`: (out, appended K row), each relative to the case's max"""
    d = dk = 0.0
    for key in keys:
        o64, k64 = attn_ref64(key)
        o32, k32 = attn_reference(attn_case(*key), np.float32)
        d = max(d, float(np.abs(o32 - o64).max() / np.abs(o64).max()))
        dk = max(dk, float(np.abs(k32 - k64).max() / np.abs(k64).max()))
    return d, dk


# ---------------------------------------------------------------- attention tolerances
# measured with d_ref() on the CPU (numpy float32 against float64): over attn_case_keys() 1.606e-6 for `out` (worst: heads 2 / 1,
# 100 rows at base 100) and 2.14e-7 for the appended K rows; over the stress cases 1.743e-6 for `out` — beyond the others' figure, so
# they get their own. The GPU bounds are therefore 6.4e-6 (stress: 7.0e-6) and 8.6e-7. test_prefill_ops_reference.py recomputes them.
D_REF = 1.61e-6
D_REF_K = 2.15e-7
D_REF_STRESS = 1.75e-6


# ---------------------------------------------------------------- prefill attention over pages
# (tests/test_gpu_prefill_paged.py; the CPU side is in test_prefill_ops_reference.py.) The same chunk as above through
# q3_attn_prefill_ex with layout = 1: the logical cache scattered over two pattern-filled slabs, the page table between them.
LONG = dict(rps=40, base=8152, n_seq=1, max_seq=8192)      # page 63 of the table, 256 key tiles, both slabs full
LONG_RATIOS = [(2, 1), (2, 2)]
LONG_KERNELS = [(GEN_T, 2), (X3, 1), (X3, 2)]               # what a prompt of >= 1024 positions runs (bf16x3, two halves) and its neighbours
SHARED = dict(rps=70, base=256, n_seq=3, pages=2)           # sequences 0 and 1 share pages 0 and 1: the prefix-cache form


def paged_max_seq(rps, base):
    """MAX_SEQ: four pages per row — every row has page edges, several rotations and pages beyond the chunk that must keep their
    bits — and the inputs of a (rps, base, n_seq) the contiguous tests also run are the very same arrays"""
    assert base + rps <= MAX_SEQ
    return MAX_SEQ


def paged_key(nh, nkv, rps, base, n_seq, stress=False, shared=0, max_seq=None):
    return (nh, nkv, rps, base, n_seq, stress, paged_max_seq(rps, base) if max_seq is None else max_seq, shared)


def paged_rows(kernel, halves, nrep):
    """(rps, base_pos, n_seq, stress, shared pages) a (kernel, halves) pair runs over pages, each against one rule of the paged path"""
    qb = query_block(kernel, nrep)
    rows = [
        (1, 127, 1, False, 0),        # the appended row is the last row of page 0
        (1, 128, 1, False, 0),        # the append opens page 1 over a wholly visible page 0
        (130, 0, 2, False, 0),        # no cache: one k_qknorm_rope_kv launch writes two pages of each row
        (33, 112, 3, False, 0),       # a chunk across the 127 / 128 edge, 3 sequences
        (qb + 1, 128, 1, False, 0),   # a second query block (one live row) behind a whole cached page
        (200, 128, 2, False, 0),      # three pages, the 255 / 256 edge inside the chunk
        (STRESS["rps"], STRESS["base"], STRESS["n_seq"], True, 0),      # sequence 1's hot key at position 127 is the last row of page 0
        (SHARED["rps"], SHARED["base"], SHARED["n_seq"], False, SHARED["pages"]),
    ]
    if kernel in (GEN_T, X3):         # the unaligned-base fix, now with a page edge inside the cache (100) and inside the first wave (130)
        rows += [(100, base, 1, False, 0) for base in UNALIGNED_BASES]
    return rows


def paged_cases():
    """every launch of the GPU file: (key, kernel, halves, n_layers, layer). The layer alternates between the cases of a ratio; the
    last case of each ratio runs on layer 3 of 4."""
    out = []
    for (nh, nkv) in RATIOS:
        nrep = nh // nkv
        mine = []
        for (kernel, halves) in attn_kernels(nrep):
            for (rps, base, n_seq, stress, shared) in paged_rows(kernel, halves, nrep):
                mine.append((paged_key(nh, nkv, rps, base, n_seq, stress, shared), kernel, halves))
        if (nh, nkv) in LONG_RATIOS:
            for (kernel, halves) in LONG_KERNELS:
                mine.append((paged_key(nh, nkv, LONG["rps"], LONG["base"], LONG["n_seq"], max_seq=LONG["max_seq"]), kernel, halves))
        for i, (key, kernel, halves) in enumerate(mine):
            n_layers, layer = (4, 3) if i == len(mine) - 1 else (2, i % 2)
            out.append((key, kernel, halves, n_layers, layer))
    return out


def paged_case_keys():
    """the distinct inputs of paged_cases(): what the D_REF recomputation and the mutation check run over"""
    keys = []
    for (key, _, _, _, _) in paged_cases():
        if key not in keys:
            keys.append(key)
    return keys


def is_long(key):
    return key[6] == LONG["max_seq"]


def case_d_ref(key):
    return D_REF_STRESS if key[5] else D_REF


def prefill_page_slots(n_seq, n_pg, n_slabs, seed, shared=None, private=False):
    """[n_seq][n_pg] slots of 0 .. 32 * n_slabs - 1, drawn from a seeded permutation: distinct, a row's pages in no order (not
    ascending when it has more than two) and — with two slabs and more than one page — on both slabs. shared = (sequences, pages):
    those sequences name the first of them's slots for their first `pages` pages (a prefix they have in common); the slots they
    would have had stay unused — private = True returns the table with those slots instead, equal everywhere else."""
    total = SLAB_SLOTS * n_slabs
    assert n_seq * n_pg <= total, "not enough slots"
    rng = np.random.default_rng(seed)

    def fine(slots):
        both = n_slabs < 2 or n_pg < 2 or all(len(set((slots[s] // SLAB_SLOTS).tolist())) == 2 for s in range(n_seq))
        return both and (n_pg <= 2 or all(not (np.diff(slots[s]) > 0).all() for s in range(n_seq)))
    for _ in range(1000):
        own = rng.permutation(total)[:n_seq * n_pg].reshape(n_seq, n_pg).astype(np.int32)
        slots = own.copy()
        if shared is not None:
            seqs, pages = shared
            assert pages <= n_pg and len(seqs) >= 2
            for s in seqs[1:]:
                slots[s, :pages] = slots[seqs[0], :pages]
        if fine(own) and fine(slots):
            return own if private else slots
    raise AssertionError("no slot table with the wanted properties")


def case_page_slots(key, private=False):
    """the slot table of a paged case (seeded by the case): two slabs; the shared-prefix case shares unless `private`"""
    nh, nkv, rps, base, n_seq, stress, max_seq, shared = key
    seed = nh * 1009 + nkv * 101 + rps * 17 + base * 3 + n_seq
    return prefill_page_slots(n_seq, max_seq // PAGE, 2, seed, ((0, 1), shared) if shared else None, private)


# --- what the bound can see: mutations of the key set, in float64
def attn_reference_mutated(c, mutation):
    """attn_reference in float64 with ONE thing wrong in the LAST sequence's keys (every head): 'drop' = the key at the last page
    edge below the chunk's end (position 0 when there is none) is left out, 'dup' = it is counted twice, 'page' = the rows of its
    page 0 come from the neighbour sequence (the next one; a sequence alone gets other random rows — what a stranger's page holds)."""
    nh, nkv, rps, base, n_seq = c["nh"], c["nkv"], c["rps"], c["base"], c["n_seq"]
    rows = n_seq * rps; nrep = nh // nkv
    dtype = np.float64
    qkv = c["qkv"]
    qr = norm_rope(qkv[:, :nh * HD].reshape(rows, nh, HD), c["qw"], c["pos"], dtype, c["max_seq"])
    kr = norm_rope(qkv[:, nh * HD:(nh + nkv) * HD].reshape(rows, nkv, HD), c["kw"], c["pos"], dtype, c["max_seq"])
    v = qkv[:, (nh + nkv) * HD:].reshape(rows, nkv, HD).astype(dtype)
    n_keys = base + rps
    edge = max(0, (n_keys - 1) // PAGE * PAGE - 1)
    keys_of = lambda s, g: (np.concatenate([c["kc"][s, g, :base].astype(dtype), kr[s * rps:(s + 1) * rps, g]], 0),
                            np.concatenate([c["vc"][s, g, :base].astype(dtype), v[s * rps:(s + 1) * rps, g]], 0))
    out = np.zeros((rows, nh, HD), dtype=dtype)
    scale = dtype(HD ** -0.5)
    kpos = np.arange(n_keys)
    stranger = np.random.default_rng(99).standard_normal((2, nkv, PAGE, HD))
    for s in range(n_seq):
        sl = slice(s * rps, (s + 1) * rps)
        for h in range(nh):
            g = h // nrep
            K, V = keys_of(s, g)
            pos_k = kpos
            if s == n_seq - 1:
                if mutation == "drop":
                    K = np.delete(K, edge, 0); V = np.delete(V, edge, 0); pos_k = np.delete(kpos, edge)
                elif mutation == "dup":
                    K = np.concatenate([K, K[edge:edge + 1]], 0); V = np.concatenate([V, V[edge:edge + 1]], 0); pos_k = np.append(kpos, edge)
                elif mutation == "page":
                    n0 = min(PAGE, n_keys)
                    K = K.copy(); V = V.copy()
                    if n_seq > 1:
                        K2, V2 = keys_of((s + 1) % n_seq, g)
                        K[:n0] = K2[:n0]; V[:n0] = V2[:n0]
                    else:
                        K[:n0] = stranger[0, g, :n0]; V[:n0] = stranger[1, g, :n0]
                else:
                    raise ValueError(mutation)
            visible = pos_k[None, :] <= (base + np.arange(rps))[:, None]
            sc = np.where(visible, (qr[sl, h] @ K.T) * scale, -np.inf)
            pr = np.exp(sc - sc.max(axis=1, keepdims=True)); pr = pr / pr.sum(axis=1, keepdims=True)
            out[sl, h] = pr @ V
    return out.reshape(rows, nh * HD)
