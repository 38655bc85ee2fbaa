"""What tests/test_gpu_prefill_ops.py rests on and a CPU can check: the frozen D_REF figures, the bound that makes the exact GEMM
check exact, the launchers' own pick for every shape of the tables (host-only: q3_gemm_path / q3_attn_prefill_path), and the
vectorised attention reference against plain loops. For tests/test_gpu_prefill_paged.py: the same D_REF recomputation over the
paged cases, the power of the bound against a wrong key set, the slot helper's properties and every refusal of the paged entry."""
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


# ---------------------------------------------------------------- prefill attention over pages (tests/test_gpu_prefill_paged.py)
def test_paged_cases_stay_under_the_frozen_d_ref():
    """the paged cases take no constant of their own: numpy float32 against float64 over paged_case_keys() does not exceed D_REF /
    D_REF_K (stress cases: D_REF_STRESS), and the long case — 8192 keys — lies well below (measured here: 9.7e-7 and 1.2e-7)"""
    keys = C.paged_case_keys()
    plain = [k for k in keys if not k[5] and not C.is_long(k)]
    stress = [k for k in keys if k[5]]
    long_ = [k for k in keys if C.is_long(k)]
    assert len(plain) + len(stress) + len(long_) == len(keys) and len(stress) == len(C.RATIOS) and len(long_) == len(C.LONG_RATIOS)
    d, dk = C.d_ref(plain); ds, dks = C.d_ref(stress); dl, dkl = C.d_ref(long_)
    print(f"paged: out {d:.3e} (D_REF {C.D_REF:.3e}), stress {ds:.3e} (D_REF_STRESS {C.D_REF_STRESS:.3e}), long {dl:.3e}; K rows {max(dk, dks, dkl):.3e}")
    assert d <= C.D_REF and ds <= C.D_REF_STRESS and dl <= C.D_REF
    assert max(dk, dks, dkl) <= C.D_REF_K


def test_paged_table_names_every_rule():
    cases = C.paged_cases()
    keys = C.paged_case_keys()
    rows = {k[2:5] for k in keys}
    assert {(1, 127, 1), (1, 128, 1), (130, 0, 2), (33, 112, 3), (200, 128, 2), (100, 100, 1), (100, 130, 1), (20, 128, 3), (70, 256, 3), (40, 8152, 1)} <= rows
    assert {k[2] for k in keys if k[3:5] == (128, 1)} >= {9, 65, 129, 257, 33, 1}          # query block + 1 of every kernel at every ratio
    for (key, kernel, halves, n_layers, layer) in cases:
        nh, nkv, rps, base, n_seq, stress, max_seq, shared = key
        assert base + rps <= max_seq <= 64 * C.PAGE and max_seq % C.PAGE == 0 and layer < n_layers
        assert (kernel, halves) in C.attn_kernels(nh // nkv)
        if C.is_long(key):
            assert (nh, nkv) in C.LONG_RATIOS and (kernel, halves) in C.LONG_KERNELS and max_seq // C.PAGE == 64 and (base + rps + 31) // 32 == 256
        if rps == 100:
            assert kernel in (GEN_T, X3)
    for ratio in C.RATIOS:          # both layers of two, and layer 3 of four once per ratio
        mine = [(c[3], c[4]) for c in cases if c[0][:2] == ratio]
        assert set(mine) == {(2, 0), (2, 1), (4, 3)} and mine.count((4, 3)) == 1
    for ratio in C.LONG_RATIOS:
        assert {(c[1], c[2]) for c in cases if c[0][:2] == ratio and C.is_long(c[0])} == set(C.LONG_KERNELS)
    # the stress case's hot key of sequence 1 sits in the last row of page 0; the shared case's pages lie wholly below its base
    assert (C.STRESS["base"] + C.STRESS["rps"] - 1) // 32 * 32 - 1 == C.PAGE - 1
    for (nh, nkv) in C.RATIOS:          # ... and carries nearly all the weight of that sequence's last row
        key = C.paged_key(nh, nkv, C.STRESS["rps"], C.STRESS["base"], C.STRESS["n_seq"], True)
        assert key in keys
        cs = C.attn_case(*key)
        o64, _ = C.attn_ref64(key)
        for g in range(nkv):
            h = g * (nh // nkv)
            assert np.abs(o64[2 * cs["rps"] - 1, h * C.HD:(h + 1) * C.HD] - cs["vc"][1, g, C.PAGE - 1]).max() < 1e-6
    assert C.SHARED["pages"] * C.PAGE <= C.SHARED["base"]
    c = C.attn_case(*C.paged_key(2, 1, C.SHARED["rps"], C.SHARED["base"], C.SHARED["n_seq"], shared=C.SHARED["pages"]))
    n = C.SHARED["pages"] * C.PAGE
    assert (c["kc"][0, :, :n] == c["kc"][1, :, :n]).all() and (c["vc"][0, :, :n] == c["vc"][1, :, :n]).all()
    assert not (c["kc"][0, :, n:] == c["kc"][1, :, n:]).any(axis=-1).any() and not (c["kc"][0, :, :n] == c["kc"][2, :, :n]).any(axis=-1).any()


def test_the_bound_sees_a_wrong_key_set():
    """for every paged case: a key left out, a key counted twice, one page taken from the neighbour sequence — each moves the float64
    `out` by more than ten times the bound the GPU file holds the kernels to"""
    worst = {}
    for key in C.paged_case_keys():
        c = C.attn_case(*key)
        o64, _ = C.attn_ref64(key)
        bound = 4 * C.case_d_ref(key)
        for mutation in ("drop", "dup", "page"):
            dev = float(np.abs(C.attn_reference_mutated(c, mutation) - o64).max() / np.abs(o64).max())
            worst[mutation] = min(worst.get(mutation, np.inf), dev / bound)
            assert dev > 10 * bound, f"{key}: '{mutation}' moves out by {dev:.3e}, bound {bound:.3e}"
    print("smallest effect of a mutation, in units of the bound:", {m: f"{v:.0f}" for m, v in worst.items()})


def test_prefill_page_slots_properties():
    """distinct slots; a row's pages on both slabs and in no order; shared exactly where asked; seeded"""
    for key in C.paged_case_keys():
        n_seq, n_pg, shared = key[4], key[6] // C.PAGE, key[7]
        s = C.case_page_slots(key)
        assert s.shape == (n_seq, n_pg) and s.dtype == np.int32 and s.min() >= 0 and s.max() < 2 * C.SLAB_SLOTS
        assert (s == C.case_page_slots(key)).all()
        for r in range(n_seq):
            assert len(set(s[r].tolist())) == n_pg and len(set((s[r] // C.SLAB_SLOTS).tolist())) == 2
            assert n_pg <= 2 or not (np.diff(s[r]) > 0).all()
        flat = s.ravel().tolist()
        if not shared:
            assert len(set(flat)) == len(flat)
        else:
            assert (s[0, :shared] == s[1, :shared]).all()
            priv = np.concatenate([s[0], s[1, shared:], s[2]]).tolist()
            assert len(set(priv)) == len(priv) == len(set(flat))
            p = C.case_page_slots(key, private=True)
            assert len(set(p.ravel().tolist())) == p.size and (p[0] == s[0]).all() and (p[2] == s[2]).all() and (p[1, shared:] == s[1, shared:]).all()
        if C.is_long(key):
            assert sorted(flat) == list(range(64))          # both slabs full
    one = C.prefill_page_slots(3, 4, 1, 5)
    assert one.max() < C.SLAB_SLOTS and len(set(one.ravel().tolist())) == 12
    assert not (C.prefill_page_slots(3, 4, 2, 5) == C.prefill_page_slots(3, 4, 2, 6)).all()


def test_paged_entry_refuses_before_a_device_is_touched():
    """Q3_INVALID_ARG (1) / Q3_UNSUPPORTED (7) for everything the paged form cannot run — slot range, the sharing rule, max_seq, the
    layer — on a machine without a GPU, where a call that passes validation ends as Q3_NO_DEVICE (5)"""
    from qwen3_tts_rs_amd import _lib
    I, U = 1, 7
    key = C.paged_key(2, 1, C.SHARED["rps"], C.SHARED["base"], C.SHARED["n_seq"], shared=C.SHARED["pages"])
    c = C.attn_case(*key)
    good = C.case_page_slots(key)

    def run(slots=good, kc=None, max_seq=None, **kw):
        ms = c["max_seq"] if max_seq is None else max_seq
        rc, rs = C.rope(ms)
        kcache = c["kc"] if kc is None else kc
        vcache = c["vc"] if max_seq is None else np.zeros((3, 1, ms, 128), np.float32)
        if max_seq is not None:
            kcache = vcache
        a = dict(layout=1, n_layers=2, layer=1, n_slabs=2, page_slots=slots, kernel=GEN_T); a.update(kw)
        try:
            q.attn_prefill_ex(c["qkv"], 3, c["base"], c["qw"], c["kw"], C.EPS, rc, rs, kcache, vcache, 2, 1, **a)
        except _lib.Q3Error as e:
            return e.status
        return 0

    def with_(r, i, v):
        s = good.copy(); s[r, i] = v
        return s
    have_gpu = _lib.lib.q3_device_count() > 0
    if not have_gpu:
        assert run() == 5 and run(slots=C.case_page_slots(key, private=True)) == 5
    assert run(slots=with_(2, 3, 64)) == I and run(slots=with_(2, 3, -1)) == I          # slot range
    assert run(slots=with_(2, 3, 32), n_slabs=1) == I
    assert run(slots=with_(2, 1, good[2, 0])) == I                                       # one row, one slot twice
    assert run(slots=with_(2, 0, good[0, 0])) == I                                       # shared below base, but the rows differ
    assert run(slots=with_(1, 2, good[0, 2])) == I                                       # page 2 reaches beyond base_pos = 256
    assert run(slots=with_(1, 1, good[0, 0])) == I                                       # page 1 of one sequence, page 0 of another
    kc = c["kc"].copy(); kc[1, 0, 255, 127] = np.nextafter(kc[1, 0, 255, 127], np.float32(9))
    assert run(kc=kc) == I                                                               # one bit of a shared page differs
    assert run(layer=2) == I and run(layer=-1) == I and run(n_layers=5, layer=4) == I and run(n_layers=0, layer=0) == I
    assert run(n_slabs=3) == I and run(n_slabs=0) == I and run(page_slots=None) == I
    assert run(layout=3) == I and run(layout=-1) == I
    assert run(layout=2) == U                                                            # bf16 pages: prefill never runs on them
    assert run(slots=np.zeros((3, 65), np.int32), max_seq=65 * 128) == I                 # beyond 64 pages of 128
    # the contiguous form is untouched by all of this
    a = _lib.CAttnPrefillEx()
    assert _lib.lib.q3_attn_prefill_ex(0, a) == I


def test_entry_refuses_a_chunk_beyond_int_range():
    """base_pos + rps is checked without forming the sum (it used to overflow int for a base_pos near INT32_MAX), and max_seq stops at
    2^20 (the page count used to round INT32_MAX up); both are Q3_INVALID_ARG before any array is read"""
    from qwen3_tts_rs_amd import _lib
    buf = np.zeros(16, np.float32)
    a = _lib.CAttnPrefillEx()
    for f in ("qkv", "q_norm_w", "k_norm_w", "rope_cos", "rope_sin", "kcache", "vcache", "out"):
        setattr(a, f, buf.ctypes.data)
    a.n_seq, a.rps, a.nh, a.nkv, a.ld_qkv, a.ld_out, a.kernel, a.halves = 1, 4, 2, 1, 512, 256, -1, 1
    for base, max_seq in ((2**31 - 1, 256), (2**31 - 4, 256), (253, 256), (0, 2**31 - 1), (0, 2**20 + 1)):
        a.base_pos, a.max_seq = base, max_seq
        assert _lib.lib.q3_attn_prefill_ex(0, a) == 1 and b"bad shape" in _lib.lib.q3_last_error(), (base, max_seq)
