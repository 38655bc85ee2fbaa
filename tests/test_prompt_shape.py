"""The prompt layout (q3_prompt_shape: PromptShape / prompt_positions of the engine, host only) against the CPU oracle and a numpy
restatement of the text projection, neither of which shares code with the engine: prefill length, trailing text rows, the frame
limit under the ICL cap, and the prompt rebuilt position by position from the entry's tables."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, synth
import oracle as O
import np_reference as NP
from common import manifest_handle, synthetic_prompt

KV_PAGE = 128


@pytest.fixture(scope="module")
def models():
    cfg = q.tiny()
    h = manifest_handle(cfg)
    om = O.OracleModel(cfg); w = NP.W()
    for name, arr, dt in synth.synthetic_checkpoint(cfg, h, synth.DEFAULT_SEED):
        if not name.startswith("decoder."):
            om.set_tensor(name, arr, dt); w.add(name, arr, dt)
    _lib.lib.q3_model_free(h)
    om.finalize(1)
    yield cfg, om, NP.NpModel(cfg, w)
    om.close()


def _grid(cfg):
    rng = np.random.default_rng(17)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)

    def ref(n):
        c = rng.integers(0, 2048, size=(n, 16)).astype(np.uint32); c[:, 0] = rng.integers(0, 3072, n)
        return c
    out = []
    for n in (0, 1, 2, 9):
        out.append((f"custom-t{n}", q.Utterance(synthetic_prompt(n, 1), q.Speaker.Vivian, q.Language.Chinese), 200))
    for ni in (0, 7, 128, 300):
        for n in (0, 1, 6):
            out.append((f"design-i{ni}-t{n}", q.Utterance(synthetic_prompt(n, 2), language=q.Language.German, instruct_ids=synthetic_prompt(ni, 50)), 200))
    for n in (0, 1, 7):
        out.append((f"xvector-t{n}", q.Utterance(synthetic_prompt(n, 3), language=q.Language.French, xvector=xv), 200))
    out.append(("codes-without-transcript", q.Utterance(synthetic_prompt(4, 3), language=q.Language.French, xvector=xv, ref_codes=ref(5)), 200))
    for n, nrt, nr in ((6, 4, 3), (2, 1, 8), (0, 3, 2), (11, 3, 5), (20, 3, 5)):
        for ml in (50, 200):
            u = q.Utterance(synthetic_prompt(n, 4), language=q.Language.Korean, xvector=xv, ref_codes=ref(nr), ref_text_ids=synthetic_prompt(nrt, 5))
            out.append((f"icl-t{n}-rt{nrt}-r{nr}-ml{ml}", u, ml))
    return out


_CASES = _grid(q.tiny())


def _row_ids(rec, u):
    """the token id of every projected text row, placed by the record's own row indices"""
    ids = [None] * rec.n_rows
    ins = list(u.instruct_ids) if u.instruct_ids is not None else []
    assert rec.n_ins == len(ins) and rec.r_role == rec.n_ins
    ids[:rec.n_ins] = ins
    ids[rec.r_role:rec.r_role + 3] = [NP.IM_START, NP.ASSISTANT, NP.NEWLINE]
    ids[rec.r_pad] = NP.TTS_PAD; ids[rec.r_bos] = NP.TTS_BOS
    text = (list(u.ref_text_ids) if rec.icl else []) + list(u.text_ids)
    ids[rec.r_text:rec.r_text + len(text)] = text
    ids[rec.r_eos] = NP.TTS_EOS
    assert len(ids) == rec.n_rows and all(i is not None for i in ids), ids
    return [int(i) for i in ids]


@pytest.mark.parametrize("name,u,max_length", _CASES, ids=[c[0] for c in _CASES])
def test_shape_against_the_oracle(models, name, u, max_length):
    cfg, om, npm = models
    opts = q.SynthesisOptions(max_length=max_length, seed=1, eos_token_id=None)
    rec, tr, ci = api.prompt_shape(u, opts, tables=True)
    s = O.OracleSession(om, u, opts)
    try:
        ref = s.prefill_embeds().astype(np.float64); otr, opad = s.trailing()
        assert rec.prefill_len == s.prefill_len() == ref.shape[0]
        assert rec.trailing_len == otr.shape[0]
        assert rec.limit == s.effective()[1]
    finally:
        s.close()
    n_text = len(u.text_ids)
    icl = u.ref_codes is not None and u.ref_text_ids is not None
    assert bool(rec.icl) == icl
    if icl:
        assert rec.limit == min(max_length, max(75, 6 * n_text))                    # lib.rs:913-929
    assert rec.prefix_pages == (len(u.instruct_ids) // KV_PAGE if u.instruct_ids is not None else 0)
    # the prompt, position by position, from the tables
    rows = npm.text_proj(_row_ids(rec, u)); H = cfg.hidden
    assert tr.min() >= 0 and tr.max() < rec.n_rows
    emb = rows[tr].copy()
    for p, c in enumerate(ci):
        if c >= 0:
            emb[p] += npm.codec_emb([int(c)])[0]
        elif c == -2:
            emb[p] += np.asarray(u.xvector, np.float64)
        elif c <= -3:
            f = np.asarray(u.ref_codes).reshape(-1, 16)[-3 - c]
            e = npm.codec_emb([int(f[0])])[0]
            for g in range(1, 16):
                e = e + npm.w.g(f"talker.code_predictor.model.codec_embedding.{g - 1}.weight", cfg.cp_vocab, H)[f[g]]
            emb[p] += e
        else:
            assert c == -1
    tol = 2e-4 * max(1.0, np.abs(ref).max())
    assert np.abs(emb - ref).max() < tol, (name, float(np.abs(emb - ref).max()))
    # the closed text's trailing rows and tts_pad, where the record says they are
    assert np.abs(rows[rec.trail_base:rec.trail_base + rec.trailing_len] - otr).max() < tol
    assert np.abs(rows[rec.r_pad] - opad).max() < tol
    # open and closed forms agree; one more trailing row per token
    if n_text >= rec.open_need:
        trail = [api.prompt_shape(u, opts, n_text=k).n_trail for k in range(rec.open_need, n_text + 1)]
        assert trail[-1] + 1 == rec.trailing_len
        assert all(b - a == 1 for a, b in zip(trail, trail[1:])), trail
    assert rec.open_need == (max(1, len(np.asarray(u.ref_codes).reshape(-1, 16)) + 1 - len(u.ref_text_ids)) if icl else 1)


def test_literal_rows():
    """numbers, so that the grid does not merely follow the oracle (the rows tests/test_ragged_batch.py asserts)"""
    o = q.SynthesisOptions(max_length=20, seed=1)
    shape = lambda u, **k: api.prompt_shape(u, o, **k)
    cv = shape(q.Utterance(synthetic_prompt(9, 0)))
    assert (cv.prefill_len, cv.n_rows, cv.trailing_len, cv.n_trail, cv.overlay, cv.limit) == (10, 15, 9, 8, 6, 20)
    assert (cv.r_role, cv.r_pad, cv.r_bos, cv.r_text, cv.r_eos, cv.trail_base) == (0, 3, 4, 5, 14, 6)
    vd = shape(q.Utterance(synthetic_prompt(6, 1), instruct_ids=synthetic_prompt(7, 51)))
    assert (vd.prefill_len, vd.n_ins, vd.overlay, vd.n_rows, vd.prefix_pages) == (16, 7, 5, 19, 0)
    big = shape(q.Utterance(synthetic_prompt(8, 2), instruct_ids=synthetic_prompt(600, 52)))
    assert (big.prefill_len, big.prefix_pages, big.r_pad) == (609, 4, 603)
    empty = shape(q.Utterance(synthetic_prompt(0, 7)))
    assert (empty.prefill_len, empty.trailing_len, empty.trail_base, empty.r_eos) == (9, 1, 5, 5)
    xv = np.zeros(8, np.float32); ref = np.zeros((5, 16), np.uint32)
    icl = q.Utterance(synthetic_prompt(11, 4), xvector=xv, ref_codes=ref, ref_text_ids=synthetic_prompt(3, 94))
    r = api.prompt_shape(icl, q.SynthesisOptions(max_length=200, seed=1))
    assert (r.icl, r.n_icl, r.prefill_len, r.trailing_len, r.limit, r.open_need, r.trail_base) == (1, 6, 15, 9, 75, 3, 11)
    assert api.prompt_shape(icl, q.SynthesisOptions(max_length=200, seed=1), n_text=20).limit == 120
    rec, tr, ci = api.prompt_shape(icl, o, tables=True)
    assert list(ci[:9]) == [-1, -1, -1, NP.CODEC_THINK, NP.CODEC_THINK_BOS, q.Language.English.token_id(), NP.CODEC_THINK_EOS, -2, NP.CODEC_PAD]
    assert list(ci[9:]) == [NP.CODEC_BOS, -3, -4, -5, -6, -7] and list(tr[9:]) == [5, 6, 7, 8, 9, 10] and list(tr[:9]) == [0, 1, 2, 3, 3, 3, 3, 3, 4]


def test_record_size_and_refusals():
    L = _lib.lib
    assert ctypes.sizeof(_lib.CPromptShape) == 18 * 4
    r = _lib.CRequest(); rec = _lib.CPromptShape()
    assert L.q3_prompt_shape(None, 0, ctypes.byref(rec), None, None, 0) == 1
    assert L.q3_prompt_shape(ctypes.byref(r), 0, None, None, None, 0) == 1
    assert L.q3_prompt_shape(ctypes.byref(r), -1, ctypes.byref(rec), None, None, 0) == 1
    r.n_ref = -1
    assert L.q3_prompt_shape(ctypes.byref(r), 0, ctypes.byref(rec), None, None, 0) == 1
    r.n_ref = 0
    assert L.q3_prompt_shape(ctypes.byref(r), 3, ctypes.byref(rec), None, None, 0) == 0 and rec.prefill_len == 10
    tr = (ctypes.c_int * 10)(); ci = (ctypes.c_int * 10)()
    assert L.q3_prompt_shape(ctypes.byref(r), 3, ctypes.byref(rec), tr, None, 10) == 1              # one table without the other
    assert L.q3_prompt_shape(ctypes.byref(r), 3, ctypes.byref(rec), tr, ci, 9) == 1 and b"9 positions" in L.q3_last_error()
    assert L.q3_prompt_shape(ctypes.byref(r), 3, ctypes.byref(rec), tr, ci, 10) == 0 and list(tr) == [0, 1, 2, 3, 3, 3, 3, 3, 4, 5]
