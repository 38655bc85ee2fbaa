"""Op-level tests of decode attention in the forms a session runs (-m gpu): one step through q3_attn_step_ex against the float64
reference of attn_step_cases.py. test_gpu_attention_op.py holds the plain form (one contiguous cache, q|k|v from a row); here:

  * the paged f32 cache — k_attn_fused<NREP, 1 | 2, false> and kv_krow of the three-launch path — at positions around page
    edges, with the pages of a row scattered over the slabs in no order, on either layer of a two-layer pool;
  * the paged bf16 cache (k_attn_fused<.., true>) and the f32 -> bf16 page conversion (k_kv_pages_to_bf16);
  * q|k|v from K-slice sums, and from the table row a folded gather picks by first-max argmax (k_attn_fused, k_attn_cp<NK, true>);
  * the code predictor's 2-token first pass (k_attn_first2), several rows per sequence on the three-launch path, the zero side job.

Checked per call: `out` and the appended K row against f64 within 4 * D_REF / 4 * D_REF_K, the appended V row bit-equal to v,
every other element of the cache bit-identical, and for paged layouts stray == 0: the entry fills every slab — the other layer,
unused slots, the padding — with a pattern, and nothing outside the cache rows may differ from it afterwards."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from attn_step_cases import (D_REF, D_REF_K, EPS, HD, RATIOS, EDGE_SPLITS, TIES, TIES_RNE, make_case, ref64, reference, rope, row_positions,
                             effective_qkv, page_slots, bf16_rne_bits, bf16_to_f32, bf16_rne_of_f64, edge_keys, deep_keys, hot_keys,
                             multirow_keys, first2_keys, gather_keys, slice_keys, zero_keys)

pytestmark = pytest.mark.gpu

WORST = {}          # form -> (out, appended row) worst deviation, printed as the module ends
SOURCES = ("qkv_part", "qkv_ssq", "qkv_K", "qkv_eps", "g_logits", "g_tok", "g_qkv_tab", "g_proj_tab", "g_x", "g_codes", "g_frame_idx", "g_code_slot")
bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
kid = lambda k: f"nh{k[0]}-nkv{k[1]}-seq{k[2]}-pos{k[3][0]}x{len(k[3])}" + (f"-rps{k[4]}" if k[4] > 1 else "") + (f"-S{k[7]}" if k[7] else "") + \
    (f"-vocab{k[8]}" if k[8] else "")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for form in sorted(WORST):
        d, dk = WORST[form]
        print(f"\nworst deviation, {form}: out {d:.3e} (bound {4 * D_REF:.3e}), appended rows {dk:.3e} (bound {4 * D_REF_K:.3e})", end="")
    print()


def _run(variant, key, n_splits=1, layout=0, krp=None, layer=0, **extra):
    c = make_case(*key)
    rc, rs = rope(c["max_seq"])
    n_seq = len(c["pos"]); n_pg = (c["max_seq"] + 127) // 128
    kw = dict(qkv=c["qkv"], rows_per_seq=c["rps"], layout=layout)
    kw.update({n: c[n] for n in SOURCES if n in c})
    if layout:
        n_slabs = 2 if (n_pg > 1 or n_seq > 32) else 1
        kw.update(n_layers=2, layer=layer, n_slabs=n_slabs, kv_row_pages=n_pg if krp is None else krp,
                  page_slots=page_slots(n_seq, n_pg, n_slabs, seed=n_seq * 100 + n_pg + c["nkv"]))
    kw.update(extra)
    return q.attn_step_ex(variant, c["pos"], c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], c["nh"], c["nkv"], n_splits, **kw)


def _check(form, what, key, res, layout=0):
    """every check of one call: returns nothing, asserts"""
    c = make_case(*key)
    o64, k64, v64 = ref64(key)
    nh, nkv, rps, B = c["nh"], c["nkv"], c["rps"], c["B"]
    out, kc, vc = res["out"], res["kcache"], res["vcache"]
    assert np.isfinite(out).all(), what
    rp = row_positions(c); seq = np.repeat(np.arange(len(c["pos"])), rps)
    k_new = kc[seq, :, rp]; v_new = vc[seq, :, rp]                      # [B][nkv][128]
    v_in = effective_qkv(c, np.float32)[:, (nh + nkv) * HD:].reshape(B, nkv, HD)
    if layout == 2:
        # the V row: RNE of v, bit for bit. The K row: RNE of the f64 row — or its neighbour where the f64 row lies within the f32
        # bound of the midpoint between the two
        assert (bf16_rne_bits(v_new) == bf16_rne_bits(v_in)).all() and (bits(v_new) & 0xffff == 0).all(), f"{what}: appended V row is not RNE(v)"
        r, ulp = bf16_rne_of_f64(k64)
        g = k_new.astype(np.float64)
        off = g != r
        near = off & (np.abs(g - r) <= ulp) & (np.abs(k64 - 0.5 * (g + r)) <= 4 * D_REF_K * np.abs(k64).max())
        assert (off == near).all(), f"{what}: {int((off & ~near).sum())} appended K elements are not RNE of the row (worst {np.abs(g - r)[off & ~near].max():.3e})"
        dev_k = float((np.abs(g - k64) - 0.5 * ulp).max() / np.abs(k64).max())          # beyond half a bf16 step: the f32 part
        o64 = reference(c, np.float64, k_rows=k_new, v_rows=v_new)[0]                   # attention over the cache as it stands now
    else:
        dev_k = float(np.abs(k_new - k64).max() / np.abs(k64).max())
        if c["kind"] == "slices":
            dev_k = max(dev_k, float(np.abs(v_new - v64).max() / np.abs(v64).max()))
        else:
            assert (bits(v_new) == bits(v_in)).all(), f"{what}: appended V row is not the v part of q|k|v"
    dev = float(np.abs(out - o64).max() / np.abs(o64).max())
    w = WORST.get(form, (0.0, 0.0)); WORST[form] = (max(w[0], dev), max(w[1], dev_k))
    print(f"{form}: {what}: out dev {dev:.3e} (bound {4 * D_REF:.3e}), appended rows dev {dev_k:.3e} (bound {4 * D_REF_K:.3e})")
    assert dev <= 4 * D_REF, f"{what}: out deviates {dev:.3e} > {4 * D_REF:.3e}"
    assert dev_k <= 4 * D_REF_K, f"{what}: appended row deviates {dev_k:.3e} > {4 * D_REF_K:.3e}"
    keep = np.ones(kc.shape[:3], dtype=bool)
    for g in range(nkv):
        keep[seq, g, rp] = False
    assert (bits(kc)[keep] == bits(c["kc"])[keep]).all(), f"{what}: K cache written outside the appended rows"
    assert (bits(vc)[keep] == bits(c["vc"])[keep]).all(), f"{what}: V cache written outside the appended rows"
    if layout:
        assert res["stray"] == 0, f"{what}: {res['stray']} elements outside the cache rows changed, the first at {res['stray_at']}"
        rot = res["rot_used"]
        assert ((rot >= 0) & (rot < 128)).all()
        if rot.shape[1] > 1:
            assert all(len(set(rot[s, :, 0].tolist())) > 1 for s in range(rot.shape[0])), f"{what}: one rotation for every page of a row"


def _paged_f32(form, variant, key, n_splits, krp=None, layer=0):
    c = make_case(*key)
    what = f"variant {variant} {kid(key)} splits={n_splits} kv_row_pages={krp} layer={layer}"
    res = _run(variant, key, n_splits, layout=1, krp=krp, layer=layer)
    _check(form, what, key, res, layout=1)
    return res


# ---------------------------------------------------------------- paged f32
@pytest.mark.parametrize("n_splits", EDGE_SPLITS)
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("key", edge_keys(), ids=kid)
def test_paged_f32_page_edges(key, variant, n_splits):
    """positions on both sides of every page edge of a 4-page row. PAGED = 1 (kv_row_pages 4), and PAGED = 2 (0: unknown, 9: more
    than the scalar form holds), which reads the same operands in the same order: the one-launch kernel must give the same bits —
    and the same bits as over one contiguous cache"""
    layer = n_splits % 2
    res = _paged_f32(f"paged f32, variant {variant}", variant, key, n_splits, krp=4, layer=layer)
    for krp in (0, 9):
        r2 = _paged_f32(f"paged f32, variant {variant}", variant, key, n_splits, krp=krp, layer=layer)
        if variant == 0:
            assert (bits(r2["out"]) == bits(res["out"])).all() and (bits(r2["kcache"]) == bits(res["kcache"])).all(), f"PAGED = 2 (kv_row_pages {krp}) differs from PAGED = 1"
    if variant == 0:
        rc_ = _run(0, key, n_splits)
        assert (bits(rc_["out"]) == bits(res["out"])).all(), "paged and contiguous outputs differ"
        assert (bits(rc_["kcache"]) == bits(res["kcache"])).all() and (bits(rc_["vcache"]) == bits(res["vcache"])).all()


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("key", deep_keys(), ids=kid)
def test_paged_f32_deep_rows(key, variant):
    """position 1023, the last row the scalar table form (8 entries) can name; positions in pages 8 and 9 of a 10-page row; and
    position 8191 — table lane 63, 64 pages from two slabs on both sides of the table — at the session's 64 splits"""
    max_seq = key[2]
    for n_splits in ((64,) if max_seq == 8192 else (1, 16) if max_seq == 1024 else (3, 64)):
        res = _paged_f32(f"paged f32, variant {variant}", variant, key, n_splits, layer=1)
        if variant == 0:
            assert (bits(_run(0, key, n_splits)["out"]) == bits(res["out"])).all(), "paged and contiguous outputs differ"


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("key", hot_keys(), ids=kid)
def test_paged_f32_softmax_stress(key, variant):
    """one key ~60 logits above the rest, in the last row of page 0 (position 127) and in the first row of page 1 (128)"""
    c = make_case(*key); o64 = ref64(key)[0]
    nrep = c["nh"] // c["nkv"]
    for b, hp in enumerate(c["hot"]):
        for g in range(c["nkv"]):
            assert np.abs(o64[b, g * nrep * HD:(g * nrep + 1) * HD] - c["vc"][b, g, hp]).max() < 1e-6      # the hot key carries the weight
    for n_splits in EDGE_SPLITS:
        _paged_f32(f"paged f32, variant {variant}", variant, key, n_splits, layer=n_splits % 2)


# ---------------------------------------------------------------- paged bf16
@pytest.mark.parametrize("krp", [4, 0])
@pytest.mark.parametrize("key", edge_keys("bf16"), ids=kid)
def test_paged_bf16_page_edges(key, krp):
    c = make_case(*key)
    v = c["qkv"][:, (c["nh"] + c["nkv"]) * HD:]
    assert (v[:, :len(TIES)] == TIES).all() and (bf16_to_f32(bf16_rne_bits(TIES)) == TIES_RNE).all()          # the ties are in, and are ties
    for n_splits in EDGE_SPLITS:
        what = f"bf16 {kid(key)} splits={n_splits} kv_row_pages={krp}"
        _check("paged bf16, variant 0", what, key, _run(0, key, n_splits, layout=2, krp=krp, layer=n_splits % 2), layout=2)


def test_kv_pages_to_bf16():
    """3 pages x 2 layers x (K, V) x 2 kv heads between slots of different rotations: every element RNE of its input, nothing else
    of the destination slab touched"""
    rng = np.random.default_rng(77)
    src = rng.standard_normal((3, 2, 2, 2, 128, 128)).astype(np.float32)
    special = np.concatenate([TIES, np.array([0.0, -0.0, 3.3895314e38, -3.3895314e38, 1.17549435e-38, -1.17549435e-38], dtype=np.float32)])
    flat = src.reshape(-1)
    at = rng.permutation(flat.size)[:special.size * 40].reshape(40, -1)
    for a in at:
        flat[a] = special
    flat[:special.size] = special
    dst, stray, stray_at, rot = q.kv_pages_to_bf16_ex(src, [3, 17, 30], [28, 9, 2])
    assert (rot[0] != rot[1]).all(), "source and destination rotations coincide"
    assert stray == 0, f"{stray} elements of the destination slab outside the pages changed, the first at {stray_at}"
    want = bf16_rne_bits(src)
    assert (dst == want).all(), f"{int((dst != want).sum())} elements are not RNE of their input"


# ---------------------------------------------------------------- several rows per sequence
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("key", multirow_keys(), ids=kid)
def test_rows_per_seq(key, layout):
    """row r of a sequence sits at base + r and sees the rows the same step appended before it (base 0: nothing else; base 126:
    the step's rows lie on both sides of a page edge)"""
    for n_splits in (1, 16):
        what = f"variant 1 {kid(key)} layout={layout} splits={n_splits}"
        _check(f"rows_per_seq, variant 1, layout {layout}", what, key, _run(1, key, n_splits, layout=layout, layer=1), layout=layout)


# ---------------------------------------------------------------- the 2-token first pass
@pytest.mark.parametrize("kind", ["plain", "tok"])
@pytest.mark.parametrize("key", first2_keys(), ids=kid)
def test_first2(key, kind):
    key = key[:5] + (kind,) + key[6:8] + (64 if kind == "tok" else 0,) + key[9:]
    c = make_case(*key)
    res = _run(3, key)
    _check(f"first2{' + g_tok' if kind == 'tok' else ''}", f"variant 3 {kid(key)} {kind}", key, res)
    nh, nkv = c["nh"], c["nkv"]; nrep = nh // nkv
    v0 = c["qkv"][0::2, (nh + nkv) * HD:].reshape(-1, nkv, HD)
    o0 = res["out"][0::2].reshape(-1, nh, HD)
    for h in range(nh):
        assert (bits(o0[:, h]) == bits(v0[:, h // nrep])).all(), "row 0 (one key) is not its own V row"
    if kind == "tok":
        _check_gx(c, res, c["g_tok"])


def _check_gx(c, res, rows):
    gx = res["g_x"]; pd = c["g_proj_dim"]
    assert (bits(gx[:, :pd]) == bits(c["g_proj_tab"][rows])).all(), "g_x is not the table's residual row"
    assert (bits(gx[:, pd:]) == bits(c["g_x"][:, pd:])).all(), "g_x written beyond g_proj_dim"


# ---------------------------------------------------------------- the folded gather
def _gather(variant, key):
    c = make_case(*key)
    res = _run(variant, key)
    _check(f"gather, variant {variant}", f"variant {variant} {kid(key)}", key, res)
    rows = np.argmax(c["g_logits"], axis=1)                 # the first maximum
    assert rows[0] == 0 and rows[1] == key[8] - 1 and rows[4] == 0            # the designs do what they claim
    assert rows[2] == min(5, key[8] - 1) and rows[3] == (1029 if key[8] > 3 else 1)          # a duplicated maximum: the lower index
    assert (c["g_logits"][2] == c["g_logits"][2].max()).sum() >= 1 and (c["g_logits"][3] == c["g_logits"][3].max()).sum() == 2
    _check_gx(c, res, rows)
    want = c["g_codes"].copy(); fi = c["g_frame_idx"]
    for b in range(c["B"]):
        if fi[b] < c["g_max_frames"]:
            want[b, fi[b], c["g_code_slot"]] = rows[b]
    assert fi[-1] == c["g_max_frames"] and (res["g_codes"] == want).all(), "g_codes: a wrong code, or a write beside the frame's slot"


@pytest.mark.parametrize("key", gather_keys(0), ids=kid)
def test_gather_fused(key):
    _gather(0, key)


@pytest.mark.parametrize("key", gather_keys(2), ids=kid)
def test_gather_cp(key):
    _gather(2, key)


# ---------------------------------------------------------------- q|k|v from slice sums
@pytest.mark.parametrize("key", slice_keys(0), ids=kid)
def test_slices_fused(key):
    assert make_case(*key)["qkv"] is None                  # the kernel must not read the row buffer: there is none
    _check("slice sums, variant 0", f"variant 0 {kid(key)}", key, _run(0, key, 16))


@pytest.mark.parametrize("key", slice_keys(0, True), ids=kid)
def test_slices_fused_paged(key):
    _check("slice sums, variant 0, paged", f"variant 0 paged {kid(key)}", key, _run(0, key, 3, layout=1, layer=1), layout=1)


@pytest.mark.parametrize("key", slice_keys(2), ids=kid)
def test_slices_cp(key):
    _check("slice sums, variant 2", f"variant 2 {kid(key)}", key, _run(2, key))


# ---------------------------------------------------------------- the zero side job
@pytest.mark.parametrize("variant,key", list(zip((0, 2, 3), zero_keys())), ids=["fused", "cp", "first2"])
def test_zero_job(variant, key):
    c = make_case(*key)
    plain = _run(variant, key)
    for zero_n in (4, 1024 * c["B"]):
        buf = np.full(zero_n + 64, 3.25, dtype=np.float32)
        res = _run(variant, key, zero_buf=buf, zero_n=zero_n)
        assert (bits(res["zero_buf"][:zero_n]) == 0).all(), "the zero job left something"
        assert (bits(res["zero_buf"][zero_n:]) == bits(buf[zero_n:])).all(), "the zero job wrote beyond zero_n"
        for n in ("out", "kcache", "vcache"):
            assert (bits(res[n]) == bits(plain[n])).all(), f"{n} differs with the zero job"
    _check(f"zero job, variant {variant}", f"variant {variant} {kid(key)}", key, plain)
