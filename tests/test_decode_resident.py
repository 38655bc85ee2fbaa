"""The residency cap of the vocoder's matrix-core launches (-m gpu): ConvArgs::resident pads a launch's dynamic LDS so that at most
n of its workgroups fit a CU, which is how q3_session_run decodes finished segments BESIDE the frame loop and still leaves every CU
room for a frame workgroup (Q3_DECODE_RESIDENT). The kernels do not change, so no bit may change:

  * op level — one launch of k_conv_bf16x3 / k_resunit_bf16x3 with resident 0, 1 and 2 gives equal outputs; the launch with
    resident 1 asks for more than 64 KB (the hipFuncSetAttribute path) and succeeds;
  * end to end on the full-size codec — run() with segments decoded beside the frames under every cap equals the whole-utterance
    decode of the same codes bit for bit, EOS off and with rows that end at different frames;
  * Q3_DECODE_OVERLAP=0 is the serial path.

The fused residual unit is only ever launched at L >= 4096 (resunit_pick refuses shorter tensors, asserted below), so its cases
run at L = 4173 = 32 full time tiles + a ragged one instead of 130: the smallest length at which that launch exists."""
import re

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, synth
from common import synthetic_prompt

pytestmark = pytest.mark.gpu

CONV, TCONV, UNIT = 0, 1, 2
CU_LDS, GRANULE = 160 * 1024, 1280


def _cap_bytes(n):
    """the smallest whole number of LDS granules of which n + 1 do not fit a CU"""
    return -(-(CU_LDS // (n + 1) + 1) // GRANULE) * GRANULE


def _snake(rng, n):
    return (rng.uniform(0.5, 1.5, n).astype(np.float32), rng.uniform(0.5, 1.5, n).astype(np.float32))


# (id, kind, cin, cout, L, k, dil, stride, residual, dynamic LDS of the uncapped launch)
#   96 co x 128 t tiles, six waves: two time tiles, the second ragged; 64 co x 64 t tiles: three time tiles; the 1x1 with its
#   in-place residual (PRE); one two-tap phase pair of a transposed conv
CONV_CASES = [
    ("k7_d9_32to96_L130", CONV, 32, 96, 130, 7, 9, 1, False, 3 * (128 + 54) * 80),
    ("k7_d1_64to128_L129", CONV, 64, 128, 129, 7, 1, 1, False, 3 * (64 + 6) * 80),
    ("k1_resid_128to96_L65", CONV, 128, 96, 65, 1, 1, 1, True, 3 * 128 * 80),
    ("tconv_2taps_32to96_L130", TCONV, 32, 96, 130, 4, 1, 2, False, 3 * (128 + 1) * 80),
]


def _conv_launch(case, resident):
    _, kind, cin, cout, L, k, dil, stride, resid, _ = case
    rng = np.random.default_rng(1234)
    x = rng.standard_normal((cin, L)).astype(np.float32)
    w = (rng.standard_normal((cin, cout, k) if kind == TCONV else (cout, cin, k)) / np.sqrt(cin * k)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    n_out = cout * L * stride
    y = rng.standard_normal(n_out).astype(np.float32) if resid else np.full(n_out, np.nan, np.float32)
    y2 = np.full(n_out, np.nan, np.float32)
    kw = dict(dil=dil, stride=stride, b=b, post=_snake(rng, cout), y=y, y2=y2, resident=resident)
    if resid:
        kw["resid_in_place"] = True
    return q.conv_ex(kind, x, w, **kw)


@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_conv_cap_changes_no_bit(case):
    plain_lds = case[-1]
    y0, z0, p0, l0 = _conv_launch(case, 0)
    assert 5 <= (p0 & 31) <= 11, q.conv_path_name(p0)           # a k_conv_bf16x3 geometry: the dynamic-LDS path
    assert l0 == plain_lds                                      # resident 0: the launch as it always was
    assert np.isfinite(y0).all() and np.isfinite(z0).all() and np.abs(y0).max() > 0
    for n in (1, 2):
        y, z, p, lds = _conv_launch(case, n)
        assert p == p0
        assert lds == max(plain_lds, _cap_bytes(n)) and (n + 1) * lds > CU_LDS >= n * lds
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(z, z0)
    # resident 1 is a launch above 64 KB: it needs the kernel's dynamic-LDS limit raised, and it ran (the results above are its own)
    assert _cap_bytes(1) > 64 * 1024 and _conv_launch(case, 1)[3] == _cap_bytes(1)


@pytest.mark.parametrize("dil", [1, 9])
def test_resunit_cap_changes_no_bit(dil):
    C, L = 96, 4096 + 77
    assert q.resunit_path(C, 130, dil) == 0 and q.resunit_path(C, 4095, dil) == 0      # never launched below L = 4096
    rng = np.random.default_rng(77 + dil)
    x = rng.standard_normal((C, L)).astype(np.float32)
    w = (rng.standard_normal((C, C, 7)) / np.sqrt(C * 7)).astype(np.float32)
    w2 = (rng.standard_normal((C, C)) / np.sqrt(C)).astype(np.float32)
    b, b2 = rng.standard_normal(C).astype(np.float32), rng.standard_normal(C).astype(np.float32)
    mid, post = _snake(rng, C), _snake(rng, C)
    raw = rng.standard_normal(C * L).astype(np.float32)
    plain_lds = max(3 * (128 + 6 * dil) * 80, 3 * 32 * (C * 2 + 16))

    def launch(n):
        y, y2 = raw.copy(), np.full(C * L, np.nan, np.float32)
        return q.conv_ex(UNIT, x, w, dil=dil, b=b, w2=w2, b2=b2, mid=mid, post=post, y=y, y2=y2, resident=n)

    y0, z0, p0, l0 = launch(0)
    assert (p0 & 31) == 15 and l0 == plain_lds                  # k_resunit_bf16x3<3, 3>
    assert np.isfinite(y0).all() and np.isfinite(z0).all() and not np.array_equal(y0, raw)
    for n in (1, 2):
        y, z, p, lds = launch(n)
        assert p == p0 and lds == _cap_bytes(n) > plain_lds
        np.testing.assert_array_equal(y, y0)
        np.testing.assert_array_equal(z, z0)
    assert _cap_bytes(1) > 64 * 1024


def test_cap_refuses_static_lds_kernels():
    """k_lin_small_bf16x3 and the f32 fallbacks keep their tiles in static LDS: there is nothing to cap, and the entry says so."""
    x = np.ones((1024, 20), np.float32)
    with pytest.raises(_lib.Q3Error, match="no dynamic LDS"):
        q.conv_ex(CONV, x, np.ones((64, 1024, 1), np.float32), resident=1)


# ---- end to end: the smallest model whose codec is full size (tiny talker, production vocoder) ----
@pytest.fixture(scope="module")
def full_codec_model():
    t = q.tiny()
    cfg = q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads,
                     n_kv_heads=t.n_kv_heads, cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers,
                     cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads, name="tiny-lm-full-decoder")
    m = q.Qwen3TTS.from_synthetic(cfg, seed=synth.DEFAULT_SEED)
    yield m
    m.close()


def _utts():
    return [q.Utterance(synthetic_prompt(4 + i, i), q.Speaker.Ryan, q.Language.English, seed=42 + i) for i in range(3)]


def _opts(eos):
    if eos:
        return q.SynthesisOptions(max_length=80, temperature=1.3, top_k=0, top_p=1.0, seed=11, min_new_tokens=2)
    return q.SynthesisOptions(max_length=80, seed=11, eos_token_id=None)


_whole = {}


def _reference(gm, eos):
    """codes and whole-utterance PCM of every row, computed once per EOS case by the serial pieces (generate, then q3_session_decode)"""
    if eos not in _whole:
        s = gm.session(_utts(), _opts(eos))
        s.prefill(); s.generate(80)
        _whole[eos] = [(s.codes(b).copy(), s.decode(b).copy()) for b in range(3)]
        s.close()
        for c, p in _whole[eos]:
            c.setflags(write=False); p.setflags(write=False)
    return _whole[eos]


@pytest.mark.parametrize("eos", [False, True])
@pytest.mark.parametrize("resident", [0, 1, 2])
def test_run_capped_overlap_is_exact(full_codec_model, resident, eos, monkeypatch, capfd):
    gm = full_codec_model
    ref = _reference(gm, eos)
    for k, v in (("Q3_DECODE_OVERLAP", "1"), ("Q3_DECODE_SEG", "16"), ("Q3_DECODE_TAIL", "16"), ("Q3_DECODE_RESIDENT", str(resident)),
                 ("Q3_DECODE_LOG", "1")):
        monkeypatch.setenv(k, v)
    s = gm.session(_utts(), _opts(eos))
    capfd.readouterr()
    audio, timing = s.run()
    log = capfd.readouterr().err
    lens = [len(s.codes(b)) for b in range(3)]
    assert timing.generation_frames == sum(lens)
    if not eos:
        assert lens == [80, 80, 80]
    # the overlapped path ran, with this cap, and handed segments to the decode stream while frames were left to generate
    m = re.search(r"q3_session_run overlap: resident (\d) seg (\d+) tail (\d+), (\d+) dispatches", log)
    assert m, log
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (resident, 16, 16)
    if max(lens) > 32:
        assert int(m.group(4)) >= 1
    for b in range(3):
        np.testing.assert_array_equal(s.codes(b), ref[b][0])
        full = s.decode(b)
        assert audio[b].samples.shape == full.shape == (lens[b] * 1920,)
        np.testing.assert_array_equal(audio[b].samples, full)
        np.testing.assert_array_equal(full, ref[b][1])
    s.close()


def test_overlap_off_is_the_serial_path(full_codec_model, monkeypatch, capfd):
    gm = full_codec_model
    ref = _reference(gm, False)
    for k, v in (("Q3_DECODE_OVERLAP", "0"), ("Q3_DECODE_SEG", "16"), ("Q3_DECODE_TAIL", "16"), ("Q3_DECODE_RESIDENT", "1"), ("Q3_DECODE_LOG", "1")):
        monkeypatch.setenv(k, v)
    s = gm.session(_utts(), _opts(False))
    capfd.readouterr()
    audio, timing = s.run()
    assert "q3_session_run overlap" not in capfd.readouterr().err      # no segment went beside the frames
    assert timing.generation_frames == 3 * 80
    for b in range(3):
        np.testing.assert_array_equal(s.codes(b), ref[b][0])
        np.testing.assert_array_equal(audio[b].samples, ref[b][1])
    s.close()
