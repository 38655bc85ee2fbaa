"""What tests/test_gpu_prefill_ops.py rests on and a CPU can check: the frozen D_REF figures, the bound that makes the exact GEMM
check exact, the launchers' own pick for every shape of the tables (host-only: q3_gemm_path / q3_attn_prefill_path), and the
vectorised attention reference against plain loops."""
import numpy as np

import qwen3_tts_rs_amd as q
import prefill_ops_cases as C
from prefill_ops_cases import NONE, RESID, SWIGLU, G1_SPLIT, G1_PLANES, G2, G3, VALU, GEN2, GEN_T, X3


def test_d_ref_is_what_numpy_float32_gives():
    """the frozen constants are the measured worst case: not below what this machine measures by more than the play a BLAS's
    summation order has between CPUs (25 %), and not padded (within a factor 1.5)"""
    d, dk = C.d_ref(C.attn_case_keys())
    ds, dks = C.d_ref([C.attn_stress_key(nh, nkv) for (nh, nkv) in C.RATIOS])
    print(f"D_REF {d:.3e} D_REF_K {max(dk, dks):.3e} D_REF_STRESS {ds:.3e}")
    assert d <= 1.25 * C.D_REF and C.D_REF <= 1.5 * d
    assert max(dk, dks) <= 1.25 * C.D_REF_K and C.D_REF_K <= 1.5 * max(dk, dks)
    # the stress cases lie beyond D_REF of the others, so they have a figure of their own, by the same rule
    assert ds <= 1.25 * C.D_REF_STRESS and C.D_REF <= C.D_REF_STRESS <= 1.5 * ds
    assert 4 * max(C.D_REF, C.D_REF_STRESS) <= 2e-5          # a looser figure would mean the inputs are ill-conditioned


def test_exact_inputs_keep_every_partial_sum_below_2_pow_24():
    """16 nonzero weights of +-1 per row and |x| <= XMAX: the sum of |x * w| over ANY subset of k — so every prefix, every range sum,
    every order — plus |bias| + |resid| stays below 2^24, where f32 holds every integer. Checked at the largest K of the tables, on
    the very arrays the GPU test uploads, and the prefix sums themselves on top."""
    K = max(r[2] for r in C.GEMM_SHAPES)
    assert K == 2048 and 16 * C.XMAX + 2 * (1 << 16) < (1 << 24)
    for N in (256, 512):
        x, wb, kw, ref, (xi, wi, bi, ri) = C.exact_case(130, N, K, RESID, True, True)
        assert np.abs(xi).max() <= C.XMAX and (np.abs(wi).sum(axis=1) == 16).all() and set(np.unique(wi)) == {-1, 0, 1}
        absum = np.abs(xi) @ np.abs(wi).T + np.abs(bi)[None, :] + np.abs(ri)
        assert absum.max() < (1 << 24)
        prefix = np.cumsum(xi[:8, None, :] * wi[None, :, :], axis=2)                # [8 rows][N][K]
        assert np.abs(prefix).max() + np.abs(bi).max() + np.abs(ri).max() < (1 << 24)
        assert (x[:, :K] == xi).all() and (kw["bias"] == bi).all() and (kw["resid"][:, :N] == ri).all()     # exact in f32
        assert (ref == ref.astype(np.float32).astype(np.int64)).all()


def test_gemm_pick_table():
    """the engine's own pick for every shape of the tables: (geometry, k_ranges, k_split, n_split)"""
    for (geometry, N, K, Ms, _) in C.GEMM_SHAPES:
        for M in Ms:
            for epi in (NONE, SWIGLU):
                n = C.gemm_n(geometry, N, epi)
                sw = epi == SWIGLU
                got = q.gemm_path(M, n, K, epi=epi, norm=sw, w2=sw, planes=geometry != G1_SPLIT)
                kpad = (K + 31) // 32 * 32
                nt2, nt3 = (64, 128) if sw else (128, 256)
                if geometry == G1_SPLIT:
                    want = (G1_SPLIT, 1, 1, 1)
                elif kpad % 128 == 0 and n % nt3 == 0:
                    T = (M + 127) // 128 * (n // nt3)
                    kr = 8 if (kpad // 64) % 16 == 0 else 1
                    ks = 1
                    while kr == 8 and ks < 8 and T * ks * 2 <= 256:
                        ks *= 2
                    want = (G3, kr, ks, 1)
                elif n % nt2 == 0:
                    want = (G2, 1, 1, 2 if (n // nt2) % 2 == 0 else 1)
                else:
                    want = (G1_PLANES, 1, 1, 1)
                assert got == want, f"M={M} N={n} K={K} epi={epi}: {got} != {want}"
    # the rows the GPU file reads back through `path`
    assert q.gemm_path(130, 384, 128) == (G2, 1, 1, 1) and q.gemm_path(130, 256, 1024) == (G3, 8, 8, 1)
    assert q.gemm_path(647, 2304, 128) == (G3, 1, 1, 1)
    # without planes there is one kernel; what no geometry takes is refused
    assert q.gemm_path(4224, 2048, 2048, planes=False) == (G1_SPLIT, 1, 1, 1)
    assert q.gemm_path(5, 96, 64) is None and q.gemm_path(5, 64, 36) is None and q.gemm_path(5, 64, 36, planes=False) == (G1_SPLIT, 1, 1, 1)
    assert q.gemm_path(5, 64, 64, epi=RESID, norm=True) is None and q.gemm_path(5, 64, 64, epi=SWIGLU, norm=True) is None
    assert q.gemm_path(5, 64, 64, epi=SWIGLU, w2=True) is None and q.gemm_path(5, 64, 64, epi=SWIGLU, norm=True, w2=True) == (G2, 1, 1, 1)


def test_attn_prefill_pick_table():
    for (nh, nkv) in C.RATIOS + [(8, 1), (3, 1)]:
        for halves in (1, 2):
            for planes in (False, True):
                got = q.attn_prefill_path(nh, nkv, planes, halves)
                if nh // nkv in (1, 2, 4):
                    assert got == (X3 if planes else GEN_T, halves)
                else:          # the VALU kernel's turn, and it takes ratios 1 and 2 only
                    assert got is None
    assert q.attn_prefill_path(2, 4, False) is None and q.attn_prefill_path(2, 2, False, 3) is None


def test_attention_reference_against_plain_loops():
    c = C.attn_case(4, 2, 5, 3, 2)          # two sequences of 5 rows behind 3 cached positions, two heads per kv head
    o, k = C.attn_reference(c)
    on, kn = C.attn_reference_naive(c)
    assert np.abs(o - on).max() < 1e-12 and np.abs(k - kn).max() < 1e-12
    # causality: a row does not depend on the chunk's later rows, nor on the cache beyond base
    c2 = {key: (val.copy() if isinstance(val, np.ndarray) else val) for key, val in c.items()}
    c2["qkv"][4] += 1.0; c2["qkv"][9] -= 1.0; c2["kc"][:, :, 3:] = 7.0; c2["vc"][:, :, 3:] = -7.0
    o2, _ = C.attn_reference(c2)
    assert (o2[[0, 1, 2, 3, 5, 6, 7, 8]] == o[[0, 1, 2, 3, 5, 6, 7, 8]]).all() and not (o2[4] == o[4]).all()


def test_tables_name_every_kernel_choice():
    """every geometry and every (kernel, halves) pair has rows; the query blocks are the kernels' own"""
    assert {r[0] for r in C.GEMM_SHAPES} == {G1_SPLIT, G1_PLANES, G2, G3}
    assert [C.query_block(k, 2) for k in (VALU, GEN2, GEN_T, X3)] == [8, 64, 64, 128]
    for (nh, nkv) in C.RATIOS:
        for (kernel, halves) in C.attn_kernels(nh // nkv):
            for (rps, base, n_seq) in C.attn_rows(kernel, nh // nkv):
                assert base + rps <= C.MAX_SEQ
    # the rows the table claims: an odd tile count, a single tile, a second XCD round
    assert (31 + 256 - 1) // 32 + 1 == 9 and (200 + 128 - 1) // 32 + 1 == 11 and 5 * 2 > 8
