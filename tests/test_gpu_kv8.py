"""FP8 (e4m3) talker K/V pages — KV8, DESIGN 4.2a (-m gpu): the f32 -> KV8 page converter bit for bit against the host rule,
k_attn_kv8 against float64 attention over the DEQUANTISED cache inside the bound of the bf16-page cases (attn_step_cases.D_REF), its
refusals, and a KV8 session through own queue, page budget, replace and park / resume. No test compares KV8 codes with the f32
oracle: they are not expected to be equal."""
import functools

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from attn_step_cases import D_REF, D_REF_K, EPS, HD, make_case, reference, rope, page_slots
from common import synthetic_prompt
from kv8_cases import SPLITS, STEP_KEYS, DEEP_KEY, SLICE_KEY, ZERO_KEY, quantize_rows, dequantize, e4m3_step, converter_pages

pytestmark = pytest.mark.gpu
kid = lambda k: f"nh{k[0]}-nkv{k[1]}-seq{k[2]}-pos{'_'.join(map(str, k[3]))}" + (f"-S{k[7]}" if k[7] else "")


def test_converter_bit_for_bit():
    src = converter_pages()
    codes, scales, stray, stray_at, rot = q.kv_pages_to_fp8_ex(src, [3, 40, 62], [33, 9, 50], n_slabs=2)
    assert (rot[0] != rot[1]).any(), "source and destination rotations coincide everywhere"
    assert stray == 0, f"{stray} bytes of the destination slabs outside the pages changed, the first at {stray_at}"
    wc, ws, _ = quantize_rows(src)
    assert (scales == ws).all(), np.argwhere(scales != ws)[:4]
    assert (codes == wc).all(), np.argwhere(codes != wc)[:4]


@functools.lru_cache(maxsize=None)
def _step_case(key):
    """the case's cache quantised by the host rule (what the entry is given), and float64 attention over the dequantised cache
    with the new row quantised by the same rule from the float64 K / V: (case, codes / scales, out, k64, v64)"""
    c = make_case(*key)
    kc, ks, kd = quantize_rows(c["kc"]); vc, vs, vd = quantize_rows(c["vc"])
    cd = dict(c, kc=kd, vc=vd)
    _, k64, v64 = reference(cd)
    out = reference(cd, k_rows=quantize_rows(k64)[2], v_rows=quantize_rows(v64)[2])[0]
    return c, (kc, vc, ks, vs), out, k64, v64


def _step(key, n_splits, krp=None, **extra):
    c, (kc, vc, ks, vs), o64, k64, v64 = _step_case(key)
    nh, nkv, pos = c["nh"], c["nkv"], c["pos"]
    B = len(pos); n_pg = (c["max_seq"] + 127) // 128
    rc, rs = rope(c["max_seq"])
    kw = dict(qkv=c["qkv"], n_layers=2, layer=n_splits % 2, n_slabs=2, kv_row_pages=n_pg if krp is None else krp,
              page_slots=page_slots(B, n_pg, 2, seed=B * 100 + n_pg + nkv))
    if c["kind"] == "slices":
        kw.update(qkv_part=c["qkv_part"], qkv_ssq=c["qkv_ssq"], qkv_K=c["qkv_K"], qkv_eps=c["qkv_eps"])
    kw.update(extra)
    res = q.attn_step_kv8(pos, c["qw"], c["kw"], EPS, rc, rs, kc, vc, ks, vs, nh, nkv, n_splits, **kw)
    what = f"{kid(key)} splits={n_splits} kv_row_pages={kw['kv_row_pages']}"
    out = res["out"]
    assert np.isfinite(out).all(), what
    dev = float(np.abs(out - o64).max() / np.abs(o64).max())
    print(f"kv8 {what}: out dev {dev:.3e} (bound {4 * D_REF:.3e})")
    assert dev <= 4 * D_REF, f"{what}: out deviates {dev:.3e} > {4 * D_REF:.3e}"
    bi = np.arange(B)
    # the appended V row: the host quantiser of v, bit for bit (v is an input; a slice-sum v is computed: K's rule)
    for name, x64, exact in (("K", k64, False), ("V", v64, c["kind"] != "slices")):
        codes = res[name.lower() + "codes"][bi, :, pos]; sc = res[name.lower() + "scales"][bi, :, pos]
        wc, ws, _ = quantize_rows(x64)
        if exact:
            assert (sc == ws).all() and (codes == wc).all(), f"{what}: appended V row is not the host quantiser of v"
            continue
        assert (np.abs(sc.astype(int) - ws.astype(int)) <= 1).all(), f"{what}: {name} scale byte {sc.ravel()} vs host {ws.ravel()}"
        # every dequantised element within half an e4m3 step at the STORED scale of the float64 row, plus the prologue's f32 slack
        s = np.exp2(sc.astype(np.float64) - 127.0)[..., None]
        got = dequantize(codes, sc)
        half = 0.5 * np.maximum(e4m3_step(x64 / s), e4m3_step(got / s)) * s
        over = np.abs(got - x64) - half
        assert over.max() <= 4 * D_REF_K * np.abs(x64).max(), f"{what}: appended {name} row {over.max():.3e} beyond half a step"
    # nothing but the appended rows and their scale bytes changed
    keep = np.ones(kc.shape[:3], dtype=bool); keep[bi, :, pos] = False
    for n, a in (("kcodes", kc), ("vcodes", vc), ("kscales", ks), ("vscales", vs)):
        assert (res[n][keep] == a[keep]).all(), f"{what}: {n} written outside the appended row"
    assert res["stray"] == 0, f"{what}: {res['stray']} bytes outside the cache rows changed, the first at {res['stray_at']}"
    return res


@pytest.mark.parametrize("n_splits", SPLITS)
@pytest.mark.parametrize("key", STEP_KEYS, ids=kid)
def test_kernel_against_float64(key, n_splits):
    _step(key, n_splits)


@pytest.mark.parametrize("key,n_splits,krp", [(DEEP_KEY, 8, 0), (SLICE_KEY, 3, None)], ids=["page8-one-entry-per-lane", "slice-sums"])
def test_kernel_table_form_and_slice_sums(key, n_splits, krp):
    _step(key, n_splits, krp)


def test_kernel_zero_job():
    plain = _step(ZERO_KEY, 3)
    for zero_n in (4, 1024 * 3):
        buf = np.full(zero_n + 64, 3.25, dtype=np.float32)
        res = _step(ZERO_KEY, 3, zero_buf=buf, zero_n=zero_n)
        assert (res["zero_buf"][:zero_n].view(np.uint32) == 0).all(), "the zero job left something"
        assert (res["zero_buf"][zero_n:] == buf[zero_n:]).all(), "the zero job wrote into its guard words"
        assert (res["out"].view(np.uint32) == plain["out"].view(np.uint32)).all() and (res["kcodes"] == plain["kcodes"]).all()


@pytest.mark.parametrize("extra", [dict(g_logits=np.zeros((3, 8), np.float32)), dict(rows_per_seq=2), dict(contiguous=True)],
                         ids=["g_logits", "rows_per_seq", "contiguous"])
def test_kernel_refusals(extra):
    c, (kc, vc, ks, vs), *_ = _step_case(STEP_KEYS[0])
    rc, rs = rope(c["max_seq"])
    qkv = np.repeat(c["qkv"], extra.get("rows_per_seq", 1), axis=0)
    with pytest.raises(_lib.Q3Error) as e:
        q.attn_step_kv8(c["pos"], c["qw"], c["kw"], EPS, rc, rs, kc, vc, ks, vs, c["nh"], c["nkv"], 1, qkv=qkv, n_layers=1, n_slabs=2,
                        kv_row_pages=2, page_slots=page_slots(3, 2, 2, seed=1), **extra)
    assert e.value.status == 7          # Q3_UNSUPPORTED


# ---------------------------------------------------------------- session
F = 40
OPTS = q.SynthesisOptions(max_length=F, eos_token_id=None, seed=3)
UTTS = [q.Utterance(synthetic_prompt(9, 0), q.Speaker.Ryan, q.Language.English, seed=5),
        q.Utterance(synthetic_prompt(14, 1), q.Speaker.Ryan, q.Language.English, seed=6),
        q.Utterance(synthetic_prompt(9, 2), language=q.Language.German, instruct_ids=synthetic_prompt(100, 52), seed=7)]      # 3 ragged rows


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), device=0, seed=1234)
    yield m
    m.close()


def _codes(gm, utts=UTTS, frames=F, **kw):
    s = api.Session(gm, utts, OPTS, kv_dtype="fp8", **kw); s.prefill(); s.generate(frames)
    out = [s.codes(b) for b in range(len(utts))]
    s.close()
    return out


@pytest.fixture(scope="module")
def want(gm):
    return _codes(gm)


def test_session_own_queue_budget_and_refusals(gm, want, monkeypatch):
    monkeypatch.setenv("Q3_AQL", "0")
    graph = _codes(gm)
    monkeypatch.delenv("Q3_AQL")
    for b in range(3):
        assert want[b].shape == (F, 16)
        np.testing.assert_array_equal(want[b], graph[b])                  # own queue == hipGraphLaunch
    s = gm.session(UTTS, OPTS, kv_dtype="fp8"); s.prefill()
    pages = sum(-(-(s.prefill_len(b)[0] + 1) // 128) for b in range(3))
    assert gm.kv_pool_info()["pages_in_use"] == -(-33 * pages // 128) < pages, "an f32 page is still held after the conversion"
    for dtype in (3, 2):                                                  # an unknown dtype; a known one after prefill
        with pytest.raises(_lib.Q3Error) as e:
            _lib.check(_lib.lib.q3_session_set_kv_dtype(s._h, dtype))
        assert e.value.status == 1                                        # Q3_INVALID_ARG
    s.close()
    # 4 f32 pages at frame 40 (row 2 crosses into its second page) against 4 KV8 pages = 132 / 128 of one
    gm.kv_pool_limit(3)
    try:
        s = gm.session(UTTS, OPTS)
        with pytest.raises(_lib.Q3Error) as e:
            s.prefill(); s.generate(F)
        assert e.value.status == 4                                        # Q3_KV_OVERFLOW
        s.close()
        for b, c in enumerate(_codes(gm)):
            np.testing.assert_array_equal(c, want[b])
    finally:
        gm.kv_pool_limit(0)
    assert gm.kv_pool_info()["pages_in_use"] == 0


def test_session_replace_and_park_resume(gm, want):
    solo = _codes(gm, [UTTS[2]])[0]
    s = api.Session(gm, [UTTS[0], UTTS[0]], OPTS, frame_budget=F, prompt_budget=300, kv_dtype="fp8")
    s.prefill(); s.generate(F); s.replace(1, UTTS[2]); s.generate(F)       # into a finished row
    np.testing.assert_array_equal(s.codes(1), solo); s.close()
    s = gm.session(UTTS, OPTS, kv_dtype="fp8"); s.prefill(); s.generate(10)
    p = s.park_row(1); s.generate(5); s.resume_row(1, p); s.generate(F)
    np.testing.assert_array_equal(s.codes(1), want[1]); np.testing.assert_array_equal(s.codes(0), want[0]); s.close()
    assert gm.kv_pool_info()["pages_in_use"] == 0
