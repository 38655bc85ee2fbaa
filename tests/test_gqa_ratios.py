"""Heads / kv-heads ratios 1 and 4 through the whole model (-m gpu). q3_model_create accepts ratios 1, 2 and 4, but every other
config of the suite (tiny, tiny_same_width, 0.6B, 1.7B) has ratio 2, so the NREP = 1 and NREP = 4 instances of the attention kernels
(k_attn_fused, k_attn_decode, k_attn_first2, k_attn_cp, k_attn_prefill*) ran nowhere. Two configs derived from q.tiny() run
against the oracle with the assertions and tolerances of the ratio-2 tests of test_gpu_parity.py — the same functions where
they take the model pair as an argument."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import oracle as O
from common import model_pair, synthetic_prompt, top2_margin, gqa_config
import test_gpu_parity as P

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", params=[1, 4])
def pair(request):
    cfg = gqa_config(request.param)
    assert cfg.n_heads // cfg.n_kv_heads == request.param == cfg.cp_heads // cfg.cp_kv_heads
    gm, om = model_pair(cfg, seed=1234)
    yield cfg, gm, om
    gm.close(); om.close()


@pytest.mark.parametrize("mode", ["custom", "design", "clone"])
def test_prefill_stages(pair, mode):
    P.test_prefill_stages(pair, mode, 9)


def test_teacher_forced_steps(pair):
    P.test_teacher_forced_steps(pair)


def _opts(sampling, frames=24):
    return q.SynthesisOptions(max_length=frames, seed=42, eos_token_id=None) if sampling == "default" else \
        q.SynthesisOptions(max_length=frames, temperature=0.0, seed=42, eos_token_id=None)


@pytest.mark.parametrize("sampling", ["greedy", "default"])
def test_free_run_graph_replay(pair, sampling):
    """B = 1, 24 frames replayed from the captured frame: k_attn_first2, k_attn_cp and the folded gathers at this ratio"""
    cfg, gm, om = pair
    utt = P._utts("custom", 20, hidden=cfg.hidden)
    rep, codes, ocodes = P._free_run_compare(cfg, gm, om, utt, _opts(sampling), True, f"{cfg.name}_{sampling}_1")
    assert rep["first_divergence"] is None, rep
    assert (codes == ocodes).all()


@pytest.mark.parametrize("sampling", ["greedy", "default"])
def test_free_run_nine_rows(pair, sampling):
    """B = 9: more than 8 rows, so the code predictor runs its 16-pass form; every row against its own oracle session"""
    cfg, gm, om = pair
    utts = [P._utts("custom", 11, index=i, hidden=cfg.hidden) for i in range(9)]
    opts = _opts(sampling)
    s = gm.session(utts, opts); s.prefill(); s.generate(24, use_graph=True)
    for b, utt in enumerate(utts):
        codes = s.codes(b)
        osess = O.OracleSession(om, utt, opts)
        ocodes, otl, ocl = osess.generate(capture=True)
        assert codes.shape == ocodes.shape == (24, 16)
        if not (codes == ocodes).all():          # tolerated only at an oracle near-tie, as in _free_run_compare
            f, g = np.argwhere(codes != ocodes)[0]
            margin = top2_margin(otl[f]) if g == 0 else top2_margin(ocl[f][g - 1])
            assert margin < P.MARGIN_EPS, (b, int(f), int(g), margin)
        osess.close()
    s.close()


@pytest.mark.parametrize("n_instruct,debug", [(200, True), (300, False)])
def test_voice_design_long_prompt(pair, n_instruct, debug):
    """VoiceDesign prompts of 209 / 309 positions. debug = True keeps the prefill on the chunked schedule (16 positions per pass:
    multi-row attention, k_qknorm_rope_kv + k_attn_decode + merge). Without it the 309 positions take the GEMM prefill at ratio 1;
    at ratio 4 the GEMM prefill does not apply (it handles 1- and 2-way GQA) and the engine must stay on the chunked schedule.
    Assertions of test_long_prompt_4k."""
    cfg, gm, om = pair
    utt = q.Utterance(synthetic_prompt(9, 1), language=q.Language.German, instruct_ids=synthetic_prompt(n_instruct, 7), seed=4)
    opts = q.SynthesisOptions(max_length=24, seed=4, eos_token_id=None)
    s = gm.session([utt], opts, debug=debug); s.prefill()
    osess = O.OracleSession(om, utt, opts)
    S, _ = s.prefill_len(0)
    assert S == osess.prefill_len() == n_instruct + 9
    hid = s.get(1, (cfg.hidden,)); ohid, olg = osess.prefill_out()
    assert np.abs(hid - ohid).max() <= 2e-4
    s.generate(24, use_graph=not debug)
    codes = s.codes(0); ocodes = osess.generate()
    n = min(len(codes), len(ocodes))
    assert n == len(ocodes) == len(codes) and (codes[:n] == ocodes[:n]).all()
    s.close(); osess.close()
