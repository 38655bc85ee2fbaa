"""Ragged first batch, packed prefill (-m gpu): the rows of a mixed-length session whose prompts take the GEMM path
from position 0 go through the talker layers TOGETHER, each at its own length, and every row must end with exactly the bits of
its own batch-1 session — last hidden state, first logits, first token and every code after it — while the short rows stay in the
equal-length groups. Q3_PREFILL_PACK=0 restores the grouped path; Q3_PREFILL_ROWS bounds a pack."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, synth
import oracle as O
from common import model_pair, synthetic_prompt

pytestmark = pytest.mark.gpu

assert [k for k in os.environ if k.startswith("Q3_PREFILL_") or k.startswith("Q3_GEMM_") or k == "Q3_KV_CONTIGUOUS"] == [], \
    "prefill knobs set: the rows would not take the passes this file names"

FRAMES = 12
LONG = [0, 1, 2, 3]          # the rows of _rows() that pack; 4 and 5 stay in groups


class _env:
    def __init__(self, **kw): self.kw = kw
    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        os.environ.update(self.kw)
    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None: os.environ.pop(k, None)
            else: os.environ[k] = v


def _rows(cfg):
    rng = np.random.default_rng(7)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)
    ref = rng.integers(0, 2048, size=(90, 16)).astype(np.uint32)
    greedy = q.SynthesisOptions(temperature=0.0, eos_token_id=None, max_length=20, seed=1)
    topk = q.SynthesisOptions(temperature=1.1, top_k=20, top_p=1.0, repetition_penalty=1.2, eos_token_id=None, max_length=20, seed=1)
    utts = [
        q.Utterance(synthetic_prompt(6, 1), language=q.Language.German, instruct_ids=synthetic_prompt(51, 61), seed=43),      # VoiceDesign(51): 60, f32-MFMA kernel
        q.Utterance(synthetic_prompt(8, 2), language=q.Language.German, instruct_ids=synthetic_prompt(250, 62), seed=44),     # VoiceDesign(250): 259, bf16x3 kernel
        q.Utterance(synthetic_prompt(5, 3), language=q.Language.German, instruct_ids=synthetic_prompt(300, 63), seed=45),     # VoiceDesign(300): 309
        q.Utterance(synthetic_prompt(11, 4), language=q.Language.French, xvector=xv, ref_codes=ref, ref_text_ids=synthetic_prompt(3, 94), seed=46),   # ICL, 90 reference frames
        q.Utterance(synthetic_prompt(9, 0), q.Speaker.Ryan, q.Language.English, seed=42),                                     # CustomVoice: 10 positions
        q.Utterance(synthetic_prompt(7, 5), language=q.Language.French, xvector=xv, seed=47),                                # x-vector clone
    ]
    limits = [14, 12, 16, 13, 12, 15]
    for i, (u, L) in enumerate(zip(utts, limits)):
        u.max_length = L
        if i in (1, 4): u.options = greedy
        if i in (2, 5): u.options = topk
    return utts


HOST = q.SynthesisOptions(max_length=20, eos_token_id=None, seed=1)


@pytest.fixture(scope="module")
def pair():
    cfg = q.tiny()
    gm, om = model_pair(cfg, seed=1234)
    yield cfg, gm, om
    gm.close(); om.close()


@pytest.fixture(scope="module")
def single(pair):
    """every row's batch-1 run, computed once: last hidden state and first logits after the prefill, codes and PCM after FRAMES frames"""
    cfg, gm, om = pair
    out = []
    for u in _rows(cfg):
        s1 = gm.session([u], u.options or HOST); s1.prefill()
        h = s1.get(1, (cfg.hidden,)).copy(); lg = s1.get(2, (cfg.codec_vocab,)).copy()
        s1.generate(FRAMES, use_graph=False)
        out.append(dict(h=h, lg=lg, codes=s1.codes(0).copy(), pcm=s1.decode(0).copy(), S=s1.prefill_len(0)[0]))
        s1.close()
    return out


def _run(gm, cfg, utts, use_graph=True, frames=FRAMES, states=False):
    s = gm.session(utts, HOST)
    s.prefill()
    info = s.prefill_info()
    st = [(s.get(1, (cfg.hidden,), b=b).copy(), s.get(2, (cfg.codec_vocab,), b=b).copy()) for b in range(len(utts))] if states else None
    s.generate(frames, use_graph=use_graph)
    codes = [s.codes(b).copy() for b in range(len(utts))]
    pcm = [s.decode(b).copy() for b in range(len(utts))]
    s.close()
    return info, codes, pcm, st


def test_lengths_are_in_the_packing_range(pair, single):
    S = [r["S"] for r in single]
    assert S[0] == 60 and S[1] == 259 and S[2] == 309 and 48 <= S[3] < 256 and S[4] == 10 and S[5] == 10, S
    assert q.prefill_pack_plan(S) == ([0, 0, 0, 0, -1, -1], [0, 60, 319, 628, 0, 0], 1)


@pytest.mark.parametrize("use_graph", [True, False])
def test_packed_rows_carry_their_batch1_bits(pair, single, use_graph):
    cfg, gm, om = pair
    utts = _rows(cfg)
    # the grouped path first, against the oracle: a difference after this can only come from the pack
    with _env(Q3_PREFILL_PACK="0"):
        info0, codes0, pcm0, _ = _run(gm, cfg, utts, use_graph)
    assert info0["packs"] == 0 and info0["rows_packed"] == 0 and info0["rows_grouped"] == 6 and info0["passes"] == 5, info0      # (rows 4 and 5 are one group of 10 positions)
    for b, u in enumerate(utts):
        osess = O.OracleSession(om, u, u.options or HOST)
        oc = osess.generate(); osess.close()
        np.testing.assert_array_equal(codes0[b][:FRAMES], oc[:FRAMES], err_msg=f"row {b}, grouped path, vs the oracle")
    info, codes, pcm, st = _run(gm, cfg, utts, use_graph, states=True)
    assert info["packs"] == 1 and info["rows_packed"] == 4 and info["rows_grouped"] == 2 and info["passes"] == 2, info
    assert info["max_pack_rows"] == sum(single[b]["S"] for b in LONG), info
    assert gm.kv_pool_info()["pages_in_use"] == 0
    for b in LONG:
        assert np.array_equal(st[b][0].view(np.uint32), single[b]["h"].view(np.uint32)), f"row {b}: last hidden state differs from its batch-1 prefill"
        assert np.array_equal(st[b][1].view(np.uint32), single[b]["lg"].view(np.uint32)), f"row {b}: first logits differ from its batch-1 prefill"
    for b in range(len(utts)):
        np.testing.assert_array_equal(codes[b], single[b]["codes"], err_msg=f"row {b} vs its batch-1 run")
        np.testing.assert_array_equal(pcm[b], single[b]["pcm"], err_msg=f"row {b} PCM vs its batch-1 run")
        np.testing.assert_array_equal(codes[b], codes0[b], err_msg=f"row {b}: packed vs Q3_PREFILL_PACK=0")


def test_row_budget_splits_the_pack(pair, single):
    cfg, gm, om = pair          # (`single` ran first: the GEMM path's own chunk length was read without the knob)
    with _env(Q3_PREFILL_ROWS="512"):
        info, codes, pcm, _ = _run(gm, cfg, _rows(cfg))
    assert info["packs"] >= 2 and info["rows_packed"] == 4 and info["max_pack_rows"] <= 512, info
    for b in range(6):
        np.testing.assert_array_equal(codes[b], single[b]["codes"], err_msg=f"row {b} vs its batch-1 run")


def test_a_row_that_finds_no_page_fails_the_whole_prefill(pair, single):
    cfg, gm, om = pair
    utts = _rows(cfg)
    need = [(single[b]["S"] + 1 + 127) // 128 for b in LONG]      # pages of the prompt and the first frame's position
    s = gm.session(utts, HOST)
    before = gm.kv_pool_info()["pages_in_use"]
    gm.kv_pool_limit(before + sum(need) - 1)                      # the pack's last row finds no page
    try:
        with pytest.raises(_lib.Q3Error) as e:
            s.prefill()
        assert e.value.status == 4, e.value                      # Q3_KV_OVERFLOW
        assert gm.kv_pool_info()["pages_in_use"] == before
        assert s.prefill_info()["packs"] == 0
    finally:
        gm.kv_pool_limit(0)
    s.prefill()                                                   # still un-prefilled: the same call now goes through
    assert s.prefill_info()["packs"] == 1
    s.generate(FRAMES)
    for b in range(6):
        np.testing.assert_array_equal(s.codes(b), single[b]["codes"], err_msg=f"row {b} after the retried prefill")
    s.close()
    assert gm.kv_pool_info()["pages_in_use"] == 0


def test_prefix_cache_rows_stay_out_misses_are_inserted(pair):
    cfg, gm, om = pair
    ins = [synthetic_prompt(300, 70), synthetic_prompt(260, 71), synthetic_prompt(140, 72), synthetic_prompt(400, 73)]
    utts = [q.Utterance(synthetic_prompt(6 + i, 20 + i), language=q.Language.German, instruct_ids=ins[i], seed=60 + i) for i in range(4)]
    ref = []
    for u in utts:                                                # cache off: every row's batch-1 codes
        s1 = gm.session([u], HOST); s1.prefill(); s1.generate(FRAMES, use_graph=False); ref.append(s1.codes(0).copy()); s1.close()
    gm.prefix_cache(32)
    try:
        s1 = gm.session([utts[0]], HOST); s1.prefill(); s1.close()
        assert gm.prefix_cache_info()["pages_cached"] == 300 // 128
        s = gm.session(utts, HOST); s.prefill()
        info = s.prefill_info()
        assert info["packs"] == 1 and info["rows_packed"] == 3 and info["rows_grouped"] == 1, info      # the cached row is not packed
        # what three one-row prefills would have inserted
        assert gm.prefix_cache_info()["pages_cached"] == 300 // 128 + 260 // 128 + 140 // 128 + 400 // 128
        s.generate(FRAMES)
        for b in range(4):
            np.testing.assert_array_equal(s.codes(b), ref[b], err_msg=f"row {b} vs its batch-1 run with the cache off")
        s.close()
    finally:
        gm.prefix_cache(0)
    assert gm.kv_pool_info()["pages_in_use"] == 0


def test_production_widths_0_6b():
    """real widths run k_lm_gemm3 and its split-K: the pack's GEMMs see another M than each row alone"""
    gm = q.Qwen3TTS.from_synthetic(q.qwen3_tts_0_6b(), seed=synth.DEFAULT_SEED)
    opts = q.SynthesisOptions(max_length=4, seed=3, eos_token_id=None)
    utts = [q.Utterance(synthetic_prompt(12, i), language=q.Language.German, instruct_ids=synthetic_prompt(n, 50 + i), seed=20 + i)
            for i, n in enumerate((60, 260, 300))]
    sb = gm.session(utts, opts); sb.prefill()
    info = sb.prefill_info()
    assert info["packs"] == 1 and info["rows_packed"] == 3 and info["max_pack_rows"] == 69 + 269 + 309, info
    lb = [sb.get(2, (gm.config.codec_vocab,), b=b).copy() for b in range(3)]
    sb.generate(4, use_graph=True)
    for b in range(3):
        s1 = gm.session([utts[b]], opts); s1.prefill()
        l1 = s1.get(2, (gm.config.codec_vocab,))
        assert np.array_equal(l1.view(np.uint32), lb[b].view(np.uint32)), f"row {b}: first logits differ from its batch-1 prefill"
        s1.generate(4, use_graph=False)
        assert np.array_equal(s1.codes(0), sb.codes(b)), f"row {b}: codes differ from its batch-1 run"
        s1.close()
    sb.close()
    gm.close()
