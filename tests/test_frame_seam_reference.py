"""What the op-level tests of the frame-seam kernels rest on, checked without a GPU (frame_seam_cases.py): the argmax rule, the
frame-embed reference against float64 and against its own row states, the coverage the case tables promise, the float32 norm's distance
from float64, and the refusals of the three test entries (Q3_INVALID_ARG before any device call)."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
import frame_seam_cases as C
from frame_seam_cases import F32, MF, GUARD


def _loop_argmax(v):
    bv, bi = -np.inf, None
    for i, x in enumerate(v):
        if x > bv:
            bv, bi = x, i
    return 0 if bi is None else bi


def test_argmax_rule():
    rng = np.random.default_rng(0)
    for V in (5, 300, 2048, 4096, 4100):
        for kind in C.KINDS:
            lg, want = C.argmax_logits(rng, V, kind)
            assert C.argmax_first(lg) == want == _loop_argmax(lg), (V, kind)
            if kind in ("waves", "lane"):
                hi = int(np.flatnonzero(lg == lg[want])[-1])
                assert hi > want and (V <= 256 or kind == "lane" or (want % 256) // 64 != (hi % 256) // 64)
                assert kind != "lane" or V <= 256 or (hi - want) % 256 == 0
            if kind == "nan":
                assert np.isnan(lg[:want]).sum() == 1


def test_frame_embed_cases_cover_what_they_promise():
    seen_states, shapes = set(), set()
    for (H, B, V, k) in C.FE_CASES:
        c = C.frame_embed_case(H, B, V, k)
        shapes.add((H, B)); seen_states |= {(s, int(f) - int(t)) for s, f, t in zip(c.state, c.frame_idx, c.trail_len)}
        body = c.want_codes != c.codes
        for b in range(B):
            f = int(c.frame_idx[b])
            if c.state[b] in ("live", "limit_frozen"):
                assert f < MF and set(np.flatnonzero(body[b].reshape(-1))) <= {f * 16, f * 16 + 15}
                assert c.want_codes[b, f, 0] == c.tok[b] and c.want_codes[b, f, 15] == c.last[b]
            else:
                assert not body[b].any(), (c.state[b], b)
                assert f == MF or (c.text_ready is not None and f >= c.text_ready[b])
        # float64 of the same sum agrees to float32 rounding of 17 terms
        b = B - 1
        f = int(c.frame_idx[b]); code = c.codes[b, min(f, MF - 1)].copy(); code[15] = c.last[b]
        s = C.bf16_to_f32(c.codec_emb[c.tok[b]]).astype(np.float64) + sum(C.bf16_to_f32(c.cp_embs[g, code[1 + g]]).astype(np.float64) for g in range(15))
        s += c.text_rows[c.trail_base[b] + f if f < c.trail_len[b] else c.pad_row[b]]
        assert np.max(np.abs(c.want_out[b] - s)) <= 17 * 2.0 ** -24 * np.max(np.abs(s)) * 8
    assert {h for h, _ in shapes} == {8, 256, 260, 1024} and {b for _, b in shapes} == {1, 3, 16}
    assert {v for _, _, v, _ in C.FE_CASES} == {5, 300, 2048, 4096, 4100}
    assert {s for s, _ in seen_states} == {"live", "at_max", "held", "limit_frozen"}
    assert {("live", -1), ("live", 0)} <= seen_states                               # f == trail_len - 1 and f == trail_len
    assert any(C.frame_embed_case(*k).text_ready is None for k in C.FE_CASES)


def test_cp_gather_cases_cover_what_they_promise():
    passes, sources, qkvs = set(), set(), set()
    for (name, p, source, qkv_dim) in C.CG_CASES:
        kw, bufs, want = C.cp_gather_case(name)
        passes.add(min(p, 2)); sources.add(source); qkvs.add(qkv_dim)
        assert (want[0] != bufs[0]).sum() > 0 and C.CG_H % 1024 and C.CG_PROJ % 1024
        width = kw["ld_out"] // 2
        body = want[0][GUARD:-GUARD].reshape(C.CG_B, 2 * width)
        assert (body[:, width:].view(np.uint32) == C.OUT_SENTINEL_BITS).all() and np.isfinite(body[:, :width]).all()
        if p >= 2:
            changed = np.flatnonzero(want[2] != bufs[2])
            assert len(changed) <= 3 and all((int(i) - GUARD) % 16 == p - 1 for i in changed)
    assert passes == {0, 1, 2} and sources == {"hidden", "emb", "proj"} and qkvs == {0, 4, 1540}


def test_rmsnorm_float32_reference_is_close_to_float64():
    for cols in C.RN_COLS:
        x, w, ref64, ref32 = C.rmsnorm_case(cols)
        d = C.rn_dev(ref32, ref64)
        assert 0.0 < d < 4e-7, (cols, d)


def test_seam_entries_refuse_bad_arguments_before_any_device_call():
    c = C.frame_embed_case(8, 3, 4100, 0)
    G = 4

    def fe(**over):
        a = dict(codec_emb=c.codec_emb, cp_embs=c.cp_embs, tok=c.tok, cp_logits_last=c.logits, frame_idx=c.frame_idx, max_frames=MF, text_rows=c.text_rows,
                 trail_base=c.trail_base, trail_len=c.trail_len, pad_row=c.pad_row, text_ready=c.text_ready, guard=G)
        a.update(over)
        codes = np.r_[np.zeros(G, np.uint32), a.pop("codes", c.codes).reshape(-1), np.zeros(G, np.uint32)]
        return q.frame_embed_ex(codes=codes, out=np.zeros(3 * 8 + 2 * G, F32), **a)
    big_code = c.codes.copy(); big_code[0, min(int(c.frame_idx[0]), MF - 1), 3] = 4100
    bad = [lambda: fe(tok=np.array([0, 7, 0], np.uint32)),                       # token outside codec_emb
           lambda: fe(frame_idx=np.array([0, MF + 1, 0], np.int32)), lambda: fe(frame_idx=np.array([-1, 0, 0], np.int32)),
           lambda: fe(codes=big_code),                                          # a code of the record it reads outside the table
           lambda: fe(pad_row=np.array([0, 99, 0], np.int32), trail_len=np.zeros(3, np.int32)),
           lambda: fe(trail_base=np.array([30, 0, 0], np.int32), trail_len=np.full(3, 6, np.int32), frame_idx=np.full(3, 5, np.int32))]
    kw, bufs, _ = C.cp_gather_case("pass1_emb_qkv4")

    def cg(name="pass1_emb_qkv4", **over):
        kw, bufs, _ = C.cp_gather_case(name)
        kw.update(over)
        return q.cp_gather_ex(out=bufs[0], qkv_out=bufs[1], codes=bufs[2], **kw)
    bad += [lambda: cg(tok=np.full(C.CG_B, C.CG_SEM, np.uint32)), lambda: cg("pass2_emb", pass_=16), lambda: cg(qkv_tab=np.zeros((C.CG_SEM, 6), F32)),
            lambda: cg("pass2_emb", frame_idx=np.array([0, -1, 0, 0], np.int32)), lambda: cg("pass0", last_hidden=None),
            lambda: cg("pass1_proj", proj_tab=np.zeros((C.CG_SEM, 2 * C.CG_PROJ + 4), F32))]       # a row wider than ld_out
    z = lambda n: np.zeros(n, F32)
    bad += [lambda: q.rmsnorm_ex(z(16), z(8), z(16), 2, 8, ldx=8, ldy=7), lambda: q.rmsnorm_ex(z(15), z(8), z(16), 2, 8),
            lambda: q.rmsnorm_ex(z(16), z(8), z(16), 2, 8, y_front=1), lambda: q.rmsnorm_ex(z(16), z(8), z(16), 2, 8, frame_idx=[0, 0]),
            lambda: q.rmsnorm_ex(z(16), z(8), z(16), 2, 8, x_off=-1)]
    for k, call in enumerate(bad):
        try:
            call()
        except _lib.Q3Error as e:
            assert e.status == 1, (k, str(e))
        else:
            raise AssertionError(f"bad argument {k} accepted")
    for f in (_lib.lib.q3_frame_embed_ex, _lib.lib.q3_cp_gather_ex):
        assert f(0, None) == 1
    if _lib.lib.q3_device_count() <= 0:          # good arguments reach the device and fail there: no CPU path
        for call in (fe, cg, lambda: q.rmsnorm_ex(z(16), z(8), z(16), 2, 8)):
            with pytest.raises(_lib.Q3Error) as e:
                call()
            assert e.value.status == 5
