"""What tests/test_gpu_codec_attn_ops.py rests on and a CPU can check: the frozen D_REF figures, the vectorised attention
reference against plain loops, the float32 RoPE recipe against float64, the case tables' own claims, the kernel selection of
launch_attn_c (host-only: q3_attn_c_path) and the refusal of every bad shape by the new entry points before anything is launched."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
import codec_attn_cases as C
from codec_attn_cases import HD, NH, QD, VALU, MFMA

INVALID = 1


def test_d_ref_is_what_numpy_float32_gives():
    """the frozen constants are the measured worst case of the reference in numpy float32: each measurement lies within
    [0.5, 1.0] x its constant — neither exceeded nor padded"""
    d, ds = C.d_ref()
    dsilu = C.d_ref_silu()
    print(f"D_REF {d:.3e} D_REF_STRESS {ds:.3e} D_REF_SILU {dsilu:.3e}")
    assert 0.5 * C.D_REF <= d <= C.D_REF
    assert 0.5 * C.D_REF_STRESS <= ds <= C.D_REF_STRESS
    assert 0.5 * C.D_REF_SILU <= dsilu <= C.D_REF_SILU
    assert 4 * max(C.D_REF, C.D_REF_STRESS) <= 1e-5          # a looser figure would mean the inputs are ill-conditioned


def test_attention_reference_against_plain_loops():
    qkv = C.whole_case(7, 2)
    assert np.abs(C.attn_reference(*qkv, 2) - C.attn_reference_naive(*qkv, 2)).max() < 1e-12
    assert np.abs(C.attn_reference(*qkv, 2, np.float64, 3) - C.attn_reference_naive(*qkv, 2, 3)).max() < 1e-12
    # a window that covers everything is the causal reference itself
    assert (C.attn_reference(*qkv, 2, np.float64, 7) == C.attn_reference(*qkv, 2)).all()
    # causality: a query does not depend on later columns; window 1 returns v
    q_, k, v = (a.copy() for a in qkv)
    k[:, 5:] += 3.0; v[:, 5:] -= 3.0; q_[:, 5:] *= 2.0
    o, o2 = C.attn_reference(*qkv, 2), C.attn_reference(q_, k, v, 2)
    assert (o2[:, :5] == o[:, :5]).all() and not (o2[:, 5:] == o[:, 5:]).any()
    assert np.abs(C.attn_reference(*qkv, 2, np.float64, 1) - qkv[2]).max() < 1e-15


def test_stress_cases_are_what_they_claim():
    """the hot key sits ~60 logits above the rest for the aligned query, in the key tile of the wave the case names, and no query before
    it sees it"""
    assert [j // 32 % 4 for j in C.STRESS_KEYS] == [0, 1, 3]
    base = C.whole_case(C.STRESS_L, NH)
    for j in C.STRESS_KEYS:
        q_, k, v = C.whole_case(C.STRESS_L, NH, j)
        logits = (q_[:HD, C.STRESS_HOT_QUERY].astype(np.float64) @ k[:HD].astype(np.float64)) / 8.0
        rest = np.delete(logits, j)
        assert 45.0 < logits[j] - rest.max() < 90.0
        assert (q_ == base[0]).all() and (v == base[2]).all() and (np.delete(k, j, axis=1) == np.delete(base[1], j, axis=1)).all()
        o, ob = C.whole_ref64(C.STRESS_L, NH, j), C.whole_ref64(C.STRESS_L, NH)
        assert (o[:, :j] == ob[:, :j]).all() and (o[HD:] == ob[HD:]).all()
        # the aligned query returns that key's value column, to the weight the others keep
        assert np.abs(o[:HD, C.STRESS_HOT_QUERY] - v[:HD, j]).max() < 1e-12


def test_tables_reach_what_they_name():
    """the case tables against the kernels' own tiling (32-query tiles at absolute multiples of 32, four waves over the key tiles)"""
    tiles = lambda a0, e: ((e - 1) >> 5) - (a0 >> 5) + 1
    assert [tiles(*r) for r in C.STREAM_ROWS] == [1, 1, 3, 4] and tiles(*C.STREAM_SINGLE[0]) == 3
    assert C.CAP % 32 != 0 and C.STREAM_ROWS[-1][1] == C.CAP and C.STREAM_ROWS[2][0] % 32 == 30
    assert all(e <= 192 for (_, e) in C.BLOCKED_ROWS) and C.LAYER != 0
    N, qcols = C.stream_layout(C.STREAM_ROWS)
    assert N == 1 + 1 + 40 + 104 + C.SPARE and qcols == [0, 1, 2, 42]
    caches = C.stream_caches(C.STREAM_ROWS)
    assert np.isnan(caches[:, 0]).all() and np.isnan(caches[2, 1, :, :, 70:]).all() and not np.isnan(caches[2, 1, :, :, :70]).any()
    for bf in C.BLOCK_FRAMES:
        pool, tabs, tab0, tab_n = C.blocked_pool(C.BLOCKED_ROWS, bf)
        assert tab0[0] == 0 and (tab0[1:] != 0).all() and list(tab_n) == [-(-e // bf) for (_, e) in C.BLOCKED_ROWS]
        owned = np.concatenate([tabs[t0:t0 + n] for t0, n in zip(tab0, tab_n)])
        assert len(set(owned)) == len(owned) and len(owned) == pool.shape[0] - 2          # disjoint lists, two unowned blocks
        assert list(owned) != sorted(owned)                                             # not in address order
        unowned = sorted(set(range(pool.shape[0])) - set(owned))
        assert np.isnan(pool[unowned]).all() and np.isnan(pool[:, 0]).all()
        r = 2; (a0, e) = C.BLOCKED_ROWS[r]; last = tabs[tab0[r] + tab_n[r] - 1]
        assert np.isnan(pool[last, 1, :, :, e % bf:]).all() and not np.isnan(pool[last, 1, :, :, :e % bf]).any()
    for L in C.ROPE_L:
        pos = C.rope_pos(L)
        assert pos.shape == (L,) and pos.max() == C.ROPE_NPOS - 1 > L and pos.min() >= 0
        if L > 2:
            assert (np.diff(pos) < 0).any() and (np.diff(pos) == 0).any()
    for n in C.SILU_N:
        g, _ = C.silu_case(n)
        if n > 3:
            assert g.min() == -30.0 and g.max() == 30.0 and (g == 0.0).sum() >= 2 and np.signbit(g[g == 0.0]).any() and not np.signbit(g[g == 0.0]).all()


def test_rope_float32_recipe_is_within_2_ulp_of_float64():
    """x1*c + (-x2)*s with each product and the sum rounded to float32: three roundings of half an ulp — of the products, which
    are no larger than |x| * 1 each, and of the sum — so within 2 ulp of the larger of |result|, |x1|, |x2|"""
    for L in C.ROPE_L:
        pos = C.rope_pos(L)
        for x in C.rope_case(L):
            y32 = C.rope_reference(x, pos)
            y64 = C.rope_reference(x, pos, dtype=np.float64)
            assert y32.dtype == np.float32
            half = HD // 2
            x3 = x.reshape(NH, 2, half, L)
            mag = np.maximum(np.abs(x3[:, 0]), np.abs(x3[:, 1]))                      # per (head, i, t): the larger operand
            mag = np.repeat(mag[:, None], 2, axis=1).reshape(QD, L)
            ulp = np.spacing(np.maximum(np.abs(y64), mag).astype(np.float32)).astype(np.float64)
            assert (np.abs(y32.astype(np.float64) - y64) <= 2 * ulp).all()


def test_mover_and_rvq_cases_are_consistent():
    for n in C.COPY_COLS_N:
        for Cc in C.COPY_COLS_C:
            src, dst, s_off, d_off, sp, dp, exp = C.copy_cols_case(n, Cc)
            written = ~C.is_sentinel(exp)
            assert written.sum() == n * Cc                               # disjoint destinations
            assert len(set(sp)) == n and len(set(dp)) == n and ((s_off < 0).sum() == 2 or n == 1)
            assert not written[:C.COPY_COLS_OFF[1] + C.GUARD].any() and not written[-C.GUARD:].any()
    src, dst, segs, exp = C.copy_segs_case()
    assert sorted(int(s[2]) for s in segs) == [0, 1, 256, 257] and (~C.is_sentinel(exp)).sum() == 1 + 256 + 257
    for n in C.GATHER_N:
        src, s_off, dst, exp = C.gather_case(n)
        assert (exp[n * 16:] == C.SENT_BITS).all() and s_off.max() + 16 <= src.size
    for (cb_dim, n_frames) in C.RVQ_CASES:
        frames, fcb, rest, fo, ro = C.rvq_case(cb_dim, n_frames)
        assert (frames[:, 0] >= C.CB_SIZE).all() and (frames[:, 1:] < C.CB_SIZE).all() and (frames[:, 1:] == C.CB_SIZE - 1).any()
        assert fo.shape == (cb_dim, n_frames) and ro.dtype == np.float32
        # float32 left to right is not the float64 sum rounded: the order is part of the contract
        r64 = sum(rest[i].astype(np.float64)[frames[:, 1 + i]] for i in range(15)).T
        assert np.abs(ro - r64).max() < 1e-3 * np.abs(r64).max()


def test_attn_c_path_is_host_only():
    """kernel selection of launch_attn_c answers without a GPU: the engine's pick is the MFMA kernel (the Q3_ATTN_C_VALU aid is read in
    one place, attn_c_pick), the explicit form runs what it is given and refuses everything else"""
    import os
    assert "Q3_ATTN_C_VALU" not in os.environ
    assert q.attn_c_path() == MFMA and q.attn_c_path(VALU) == VALU and q.attn_c_path(MFMA) == MFMA
    assert q.attn_c_path(2) is None and q.attn_c_path(-2) is None and q.attn_c_path(MFMA, hd=128) is None
    assert ctypes.sizeof(_lib.CAttnCEx) == 14 * 4 + 9 * 8


def _refused(call, what):
    with pytest.raises(_lib.Q3Error) as e:
        call()
    assert e.value.status == INVALID, f"{what}: status {e.value.status} ({e.value})"


def test_entry_points_refuse_bad_shapes_before_launching():
    """Q3_INVALID_ARG — not a HIP error, not a launch — for every shape the kernels could not address; checked before the device is
    touched, so it holds on a machine without a GPU"""
    z = lambda *s: np.zeros(s, np.float32)
    # whole / window
    _refused(lambda: q.attn_c_ex(0, z(2 * 32, 8), z(2 * 32, 8), nh=2, hd=32, k=z(2 * 32, 8), v=z(2 * 32, 8)), "hd != 64")
    _refused(lambda: q.attn_c_ex(0, z(QD, 8), z(QD, 8), nh=NH, k=z(QD, 8), v=z(QD, 8), kernel=2), "kernel 2")
    _refused(lambda: q.attn_c_ex(3, z(QD, 8), z(QD, 8), nh=NH, k=z(QD, 8), v=z(QD, 8), window=0), "window 0")
    _refused(lambda: q.attn_c_ex(4, z(QD, 8), z(QD, 8), nh=NH, k=z(QD, 8), v=z(QD, 8)), "mode 4")
    # stream
    cs = lambda rows, cap=64, N=8: q.attn_c_ex(1, z(QD, N), z(QD, N), nh=NH, rows=rows, caches=z(len(rows), 2, 2, QD, cap), layer=1)
    _refused(lambda: cs([(5, 5, 0)]), "e <= a0")
    _refused(lambda: cs([(5, 4, 0)]), "e < a0")
    _refused(lambda: cs([(60, 65, 0)]), "e > cap")
    _refused(lambda: cs([(0, 9, 0)]), "more new frames than columns")
    _refused(lambda: cs([(0, 4, 5)]), "qcol + n > N")
    _refused(lambda: cs([(0, 4, -1)]), "qcol < 0")
    _refused(lambda: cs([(-1, 4, 0)]), "a0 < 0")
    _refused(lambda: q.attn_c_ex(1, z(QD, 8), z(QD, 8), nh=NH, rows=[(0, 4, 0)], caches=z(1, 2, 2, QD, 64), layer=2), "layer outside layers")
    _refused(lambda: q.attn_c_ex(1, z(64, 8), z(64, 8), nh=2, hd=32, rows=[(0, 4, 0)], caches=z(1, 2, 2, 64, 64)), "stream hd != 64")
    # blocked
    cb = lambda rows, tabs, tab0, tab_n, bf=32, n_blocks=4, N=8: q.attn_c_ex(2, z(QD, N), z(QD, N), nh=NH, rows=rows, caches=z(n_blocks, 2, 2, QD, bf),
                                                                            layer=1, tabs=tabs, tab0=tab0, tab_n=tab_n)
    _refused(lambda: cb([(0, 4, 0)], [0], [0], [1], bf=48), "bf % 32 != 0")
    _refused(lambda: cb([(30, 34, 0)], [0], [0], [1]), "block list shorter than ceil(e / bf)")
    _refused(lambda: cb([(0, 4, 0)], [0, 1], [1], [2]), "block list beyond the table")
    _refused(lambda: cb([(0, 4, 0)], [4], [0], [1]), "block outside the pool")
    _refused(lambda: cb([(0, 4, 0)], [-1], [0], [1]), "negative block")
    _refused(lambda: cb([(4, 4, 0)], [0], [0], [1]), "blocked e <= a0")
    _refused(lambda: cb([(0, 4, 6)], [0], [0], [1]), "blocked columns outside N")
    # RoPE
    cs_, sn_ = z(4, 32), z(4, 32)
    _refused(lambda: q.rope_c_ex(z(QD, 5), z(QD, 5), cs_, sn_, NH), "fewer positions than columns")
    _refused(lambda: q.rope_c_ex(z(QD, 3), z(QD, 3), cs_, sn_, NH, pos=[0, 4, 1]), "pos beyond the table")
    _refused(lambda: q.rope_c_ex(z(QD, 3), z(QD, 3), cs_, sn_, NH, pos=[0, -1, 1]), "negative pos")
    # movers
    _refused(lambda: q.copy_cols_ex(z(16), z(16), 4, [0], [4], [4], [4]), "destination column leaves its buffer")
    _refused(lambda: q.copy_cols_ex(z(16), z(16), 4, [4], [0], [4], [4]), "source column leaves its buffer")
    _refused(lambda: q.copy_cols_ex(z(16), z(16), 4, [0], [0], [1], [1], dst_off=13), "dst_off pushes the column out")
    _refused(lambda: q.copy_cols_ex(z(16), z(16), 4, [-1], [-1], [1], [1]), "negative destination")
    _refused(lambda: q.copy_segs_ex(z(16), z(16), [(8, 0, 9)]), "segment leaves the source")
    _refused(lambda: q.copy_segs_ex(z(16), z(16), [(0, 8, 9)]), "segment leaves the destination")
    _refused(lambda: q.copy_segs_ex(z(16), z(16), [(0, 0, 0)]), "only empty segments")
    _refused(lambda: q.gather_frames_ex(np.zeros(32, np.uint32), [17], np.zeros(16, np.uint32)), "frame leaves the source")
    _refused(lambda: q.gather_frames_ex(np.zeros(32, np.uint32), [0, 16], np.zeros(31, np.uint32)), "destination too small")
    # RVQ / SiLU
    _refused(lambda: q.rvq_embed_ex(np.zeros((2, 16), np.uint32), z(4, 257), z(15, 4, 257), z(514), z(514)), "cb_dim > 256")
    _refused(lambda: q.rvq_embed_ex(np.zeros((2, 16), np.uint32), z(4, 8), z(15, 4, 8), z(15), z(15)), "outputs too small")
    _refused(lambda: q.rvq_embed_ex(np.zeros((2, 16), np.uint32), z(4, 8), z(15, 4, 8), z(20), z(20), out_front=8), "out_front pushes the result out")
    _refused(lambda: q.silu_mul_ex(z(8), z(8), z(7)), "y shorter than n")
