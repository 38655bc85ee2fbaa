"""What the decode-attention form tests (test_gpu_attention_forms.py) rest on, checked without a GPU: the frozen tolerance constants,
the vectorised float64 reference against plain loops, the claims of the case tables (which positions straddle a page, that the
stress key carries the weight, that the tie values are ties, that slot lists are distinct), a numpy model of the scatter / gather
through page_slots + rotation, and every refusal of q3_attn_step_ex / q3_kv_pages_to_bf16_ex before a device is touched."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
import attn_step_cases as A
from attn_step_cases import K, HD, EPS


def test_frozen_constants():
    d, dk = A.measure_d_ref()
    print(f"measured: out {d:.3e} (frozen {A.D_REF:.3e}), appended rows {dk:.3e} (frozen {A.D_REF_K:.3e})")
    assert 0.5 * A.D_REF <= d <= A.D_REF
    assert 0.5 * A.D_REF_K <= dk <= A.D_REF_K
    assert 4 * A.D_REF <= 2e-5
    # the 8192-key case alone stays below the common constant: it needs none of its own
    assert A.measure_d_ref([A.deep_keys()[-1]])[0] <= A.D_REF


def test_vectorised_reference_against_plain_loops():
    keys = [K(4, 2, 17, (0, 1, 5, 16)), K(2, 2, 17, (3,)), K(4, 1, 40, (0, 30), rps=5), K(4, 2, 17, (0, 0), rps=2, kind="tok", vocab=64),
            K(4, 2, 17, (4,) * 7, kind="gather", vocab=3), K(4, 2, 17, (7,) * 17, kind="slices", S=8), K(4, 1, 140, (126, 129))]
    for key in keys:
        c = A.make_case(*key)
        for a, b in zip(A.reference(c), A.reference_loops(c)):
            assert np.abs(a - b).max() < 1e-12, key


def test_reference_takes_rows_from_the_right_source():
    c = A.make_case(*K(4, 2, 17, (4,) * 7, kind="gather", vocab=2047))
    rows = np.argmax(c["g_logits"], axis=1)
    assert rows.tolist()[:6] == [0, 2046, 5, 1029, 0, 777] and c["qkv"] is None
    assert (A.effective_qkv(c, np.float32) == c["g_qkv_tab"][rows]).all()
    # a duplicated maximum really is duplicated, and np.argmax takes the first
    assert c["g_logits"][2, 5] == c["g_logits"][2, 1029] == c["g_logits"][2].max()
    assert c["g_logits"][3, 1029] == c["g_logits"][3, 2043] == c["g_logits"][3].max()
    assert np.isneginf(c["g_logits"][5]).sum() == 2046
    c = A.make_case(*K(4, 2, 17, (7,) * 17, kind="slices", S=2))
    x = A.effective_qkv(c, np.float64)
    want = (c["qkv_part"][0].astype(np.float64) + c["qkv_part"][1]) / np.sqrt((c["qkv_ssq"][0].astype(np.float64) + c["qkv_ssq"][1]) / 1024 + EPS)[:, None]
    assert np.abs(x - want).max() < 1e-14 and 0.5 < x.std() < 2.0
    c = A.make_case(*K(4, 2, 17, (0, 0), rps=2, kind="tok", vocab=64))
    x = A.effective_qkv(c, np.float32)
    assert (x[0::2] == c["qkv"][0::2]).all() and (x[1::2] == c["g_qkv_tab"][c["g_tok"]]).all()


def test_case_tables_claim_what_they_do():
    # page edges: the 7-row call has rows whose last cached key pair (pos - 2, pos - 1) straddles a page, rows whose new position is
    # the first or the last row of a page, and split starts that are odd next to an edge
    assert [p % 128 for p in A.EDGE_POS] == [126, 127, 0, 1, 127, 0, 127]
    # the two half-wave groups of a wave ask for keys in different pages only where a split starts on an odd position: never
    # with 1 or 3 splits of these rows; with both keys cached at (127, 128) for pos 256 in 16 and in 64 splits, and in the deep rows
    assert all(A.pairs_across_pages(p, n) == [] for p in A.EDGE_POS for n in (1, 3))
    assert A.pairs_across_pages(256, 16) == A.pairs_across_pages(256, 64) == [(127, 128), (255, 256)]
    assert A.pairs_across_pages(896, 16) == [(639, 640), (767, 768), (895, 896)] and (1023, 1024) in A.pairs_across_pages(1152, 64)
    assert (127, 128) in A.pairs_across_pages(1030, 64) and (511, 512) in A.pairs_across_pages(1152, 3)
    # the stress key carries the weight
    for key in A.hot_keys():
        c = A.make_case(*key); o64 = A.ref64(key)[0]; nrep = c["nh"] // c["nkv"]
        assert c["hot"] == (127, 128)
        for b, hp in enumerate(c["hot"]):
            for g in range(c["nkv"]):
                assert np.abs(o64[b, g * nrep * HD:(g * nrep + 1) * HD] - c["vc"][b, g, hp]).max() < 1e-6
    # the ties are ties: exactly midway between two bf16 numbers, and RNE takes the even one
    t = A.TIES.astype(np.float64)
    r, ulp = A.bf16_rne_of_f64(t)
    assert (np.abs(t - r) == 0.5 * ulp).all() and (r == A.TIES_RNE).all() and (A.bf16_to_f32(A.bf16_rne_bits(A.TIES)) == A.TIES_RNE).all()
    trunc = A.bf16_to_f32((A.TIES.view(np.uint32) >> 16).astype(np.uint16))
    half_up = A.bf16_to_f32(((A.TIES.view(np.uint32).astype(np.uint64) + 0x8000) >> 16).astype(np.uint16))
    assert (trunc != A.TIES_RNE).any() and (half_up != A.TIES_RNE).any()
    c = A.make_case(*A.edge_keys("bf16")[1])
    assert (A.bf16_round(c["kc"]) == c["kc"]).all() and (A.bf16_round(c["vc"]) == c["vc"]).all()
    assert (c["qkv"][:, (c["nh"] + c["nkv"]) * HD:][:, :len(A.TIES)] == A.TIES).all()
    # slot lists: distinct, inside the slabs, the pages of a row neither ascending nor neighbours
    for n_seq, n_pg, n_slabs in ((7, 4, 2), (2, 8, 2), (3, 10, 2), (1, 64, 2), (2, 2, 2), (64, 1, 2), (17, 1, 1)):
        s = A.page_slots(n_seq, n_pg, n_slabs, seed=n_seq * 100 + n_pg)
        assert s.shape == (n_seq, n_pg) and len(set(s.reshape(-1).tolist())) == s.size and s.min() >= 0 and s.max() < 32 * n_slabs
        if 2 < n_pg < 64:
            assert all((np.diff(row) <= 0).any() and (np.abs(np.diff(row)) > 1).all() for row in s)
    assert len(A.all_cases()) == len(set(A.all_cases())) > 80


def test_scatter_gather_model_round_trips():
    rng = np.random.default_rng(5)
    n_seq, nkv, max_seq = 3, 2, 300
    logical = rng.standard_normal((n_seq, nkv, max_seq, HD)).astype(np.float32)
    slots = A.page_slots(n_seq, 3, 1, seed=1)
    rot = rng.integers(0, 128, (n_seq, 3, nkv))
    pages = A.scatter_model(logical, slots, rot, 32)
    assert (A.gather_model(pages, slots, rot, max_seq) == logical).all()
    # a row lands where the kernels look for it, and a rotation off by one is seen
    assert (pages[slots[1, 1], 1, (130 + rot[1, 1, 1]) % 128] == logical[1, 1, 130]).all()
    assert not (A.gather_model(pages, slots, (rot + 1) % 128, max_seq) == logical).all()
    used = ~np.isnan(pages).all(axis=(1, 2, 3))
    assert sorted(np.flatnonzero(used).tolist()) == sorted(slots.reshape(-1).tolist())


def _refused(call, status, why):
    with pytest.raises(_lib.Q3Error) as e:
        call()
    assert e.value.status == status, f"{why}: status {e.value.status} ({e.value})"


def test_entry_points_refuse_before_launching():
    """Q3_INVALID_ARG (1) / Q3_UNSUPPORTED (7) — not a HIP error, not a launch — for everything the kernels could not address;
    checked before the device is touched, so it holds on a machine without a GPU"""
    assert ctypes.sizeof(_lib.CAttnStepEx) == 24 * 4 + 22 * 8
    z = lambda *s: np.zeros(s, np.float32)
    one = np.ones(128, np.float32)

    def step(variant, pos=(0,), max_seq=128, nh=4, nkv=2, n_splits=1, B=None, rps=1, qkv=True, **kw):
        n_seq = len(pos); B = n_seq * rps if B is None else B
        kc = kw.pop("kc", None)
        kc = z(n_seq, nkv, max_seq, 128) if kc is None else kc
        return q.attn_step_ex(variant, list(pos), one, one, 1e-6, z(max_seq, 64), z(max_seq, 64), kc, kc, nh, nkv, n_splits,
                              qkv=z(B, (nh + 2 * nkv) * 128) if qkv else None, B=B, rows_per_seq=rps, **kw)
    paged = dict(layout=1, n_layers=2, layer=1, n_slabs=1, kv_row_pages=1, page_slots=[[3]])
    I, U = 1, 7
    _refused(lambda: step(4), I, "variant 4")
    _refused(lambda: step(0, layout=3), I, "layout 3")
    _refused(lambda: step(0, nh=6, nkv=2), U, "heads / kv heads = 3")
    _refused(lambda: step(0, n_splits=65), I, "65 splits")
    _refused(lambda: step(0, pos=(128,)), I, "position beyond max_seq")
    _refused(lambda: step(0, pos=(-1,)), I, "negative position")
    _refused(lambda: step(1, pos=(126,), rps=3), I, "the step's rows run past max_seq")
    _refused(lambda: step(0, **dict(paged, page_slots=[[32]])), I, "slot outside the slab")
    _refused(lambda: step(0, **dict(paged, page_slots=[[-1]])), I, "negative slot")
    _refused(lambda: step(0, pos=(0, 0), **dict(paged, page_slots=[[5], [5]])), I, "one slot twice")
    _refused(lambda: step(0, max_seq=64 * 128 + 1, **dict(paged, n_slabs=2, kv_row_pages=0, page_slots=[list(range(64)) + [0]])), I, "max_seq beyond 64 pages")
    _refused(lambda: step(0, max_seq=512, **dict(paged, kv_row_pages=2, page_slots=[[0, 4, 8, 12]])), I, "kv_row_pages below the row's pages")
    _refused(lambda: step(0, **dict(paged, kv_row_pages=65)), I, "kv_row_pages 65")
    _refused(lambda: step(0, **dict(paged, n_layers=5)), I, "5 layers")
    _refused(lambda: step(0, **dict(paged, layer=2)), I, "layer outside the layers")
    _refused(lambda: step(0, **dict(paged, n_slabs=3)), I, "3 slabs")
    _refused(lambda: step(0, **dict(paged, page_slots=None)), I, "paged without page_slots")
    _refused(lambda: step(2, max_seq=17, **paged), U, "layout 1 with variant 2")
    _refused(lambda: step(3, max_seq=17, rps=2, **paged), U, "layout 1 with variant 3")
    _refused(lambda: step(2, max_seq=17, **dict(paged, layout=2)), U, "layout 2 with variant 2")
    _refused(lambda: step(1, **dict(paged, layout=2)), U, "layout 2 with variant 1")
    inexact = z(1, 2, 128, 128); inexact[0, 1, 77, 3] = np.float32(1.0 + 2.0 ** -9)
    _refused(lambda: step(0, kc=inexact, **dict(paged, layout=2)), I, "layout 2 with a value that is not exact in bf16")
    _refused(lambda: step(0, rps=2), U, "rows_per_seq with variant 0")
    _refused(lambda: step(2, max_seq=17, rps=2), U, "rows_per_seq with variant 2")
    _refused(lambda: step(1, rps=9), I, "9 rows per sequence")
    _refused(lambda: step(3, max_seq=17, rps=1), I, "variant 3 with one row per sequence")
    _refused(lambda: step(3, max_seq=17, rps=3), I, "variant 3 with three rows per sequence")
    _refused(lambda: step(3, pos=(1,), max_seq=17, rps=2), I, "variant 3 from a cache that is not empty")
    _refused(lambda: step(2, pos=(16,), max_seq=17), U, "variant 2 at position 16")
    _refused(lambda: step(2, pos=(3,), max_seq=17, n_splits=2), U, "variant 2 with two splits")
    _refused(lambda: step(2, pos=(3,), max_seq=256), U, "variant 2 with max_seq 256")
    _refused(lambda: step(2, pos=(3, 4), max_seq=17), I, "variant 2 with two positions")
    part, ssq = z(2, 1, 8 * 128), np.ones((2, 1), np.float32)
    _refused(lambda: step(1, qkv=False, qkv_part=part, qkv_ssq=ssq, qkv_K=1024), I, "slice sums with variant 1")
    _refused(lambda: step(0, qkv=False, qkv_part=z(9, 1, 8 * 128), qkv_ssq=np.ones((9, 1), np.float32), qkv_K=1024), I, "9 slices")
    _refused(lambda: step(0, qkv=False, qkv_part=part, qkv_ssq=ssq, qkv_K=0), I, "slice sums without K")
    _refused(lambda: step(0, qkv=False), I, "no source of q|k|v")
    g = dict(g_qkv_tab=z(8, 8 * 128), g_proj_tab=z(8, 16), g_x=z(1, 16), g_codes=np.zeros((1, 2, 16), np.uint32), g_frame_idx=[0])
    _refused(lambda: step(1, g_logits=z(1, 8), **g), I, "g_logits with variant 1")
    _refused(lambda: step(0, g_tok=[0], **g), I, "g_tok with variant 0")
    _refused(lambda: step(0, qkv=False, g_logits=z(1, 8), qkv_part=part, qkv_ssq=ssq, qkv_K=1024, **g), I, "gather and slice sums")
    _refused(lambda: step(0, g_logits=z(1, 8), **dict(g, g_proj_tab=z(8, 18), g_x=z(1, 20))), I, "g_proj_dim not a multiple of 4")
    _refused(lambda: step(0, g_logits=z(1, 8), **dict(g, g_x=z(1, 12))), I, "g_ldx below g_proj_dim")
    _refused(lambda: step(0, g_logits=z(1, 8), **dict(g, g_frame_idx=[-1])), I, "negative frame index")
    _refused(lambda: step(0, g_logits=z(1, 8), g_code_slot=16, **g), I, "code slot 16")
    _refused(lambda: step(3, max_seq=17, rps=2, g_tok=[8], **g), I, "g_tok outside the table")
    _refused(lambda: step(0, zero_buf=z(10), zero_n=6), I, "zero_n not a multiple of 4")
    _refused(lambda: step(1, zero_buf=z(8), zero_n=8), I, "zero job on the three-launch path")
    # the page conversion
    src = z(2, 1, 2, 1, 128, 128)
    _refused(lambda: q.kv_pages_to_bf16_ex(src, [0, 0], [1, 2]), I, "one source slot twice")
    _refused(lambda: q.kv_pages_to_bf16_ex(src, [0, 1], [2, 2]), I, "one destination slot twice")
    _refused(lambda: q.kv_pages_to_bf16_ex(src, [0, 32], [1, 2]), I, "slot outside the slab")
    _refused(lambda: q.kv_pages_to_bf16_ex(z(1, 5, 2, 1, 128, 128), [0], [1]), I, "5 layers")
    _refused(lambda: q.kv_pages_to_bf16_ex(z(1, 1, 2, 9, 128, 128), [0], [1]), I, "9 kv heads")
    _refused(lambda: q.kv_pages_to_bf16_ex(z(33, 1, 2, 1, 128, 128), list(range(33)), list(range(33))), I, "33 pages")
    L = _lib.lib
    assert L.q3_kv_pages_to_bf16_ex(0, 1, 1, 1, None, None, None, None, None, None) == 1 and L.q3_attn_step_ex(0, None) == 1
    assert L.q3_attn_step_ex(0, ctypes.byref(_lib.CAttnStepEx())) == 1
