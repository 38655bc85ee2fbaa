"""Op-level tests of the frame-seam kernels (-m gpu): ONE launch per call through q3_frame_embed_ex, q3_cp_gather_ex and q3_rmsnorm_ex.
Inputs, case tables and references are in frame_seam_cases.py; what needs no GPU is in test_frame_seam_reference.py.

k_frame_embed and k_cp_gather: outputs bit-equal to the float32 restatement (bf16 -> f32 exact, adds rounded one by one, left to right),
codes bit-identical except the slots a live, ready row records, sentinels around and between the rows intact. A row that k_sample froze
at limit < max_frames is live to these kernels: it records into frame `limit` of its own block, which no reader of the codes reaches
(they stop at the row's committed count) — pinned down here as the "limit_frozen" state.
k_rmsnorm / k_rmsnorm_hold against float64: the bound is 4 x the deviation of the same formula in float32 numpy on the same inputs;
held rows keep their old output bit for bit.

Measured on an MI355X, worst deviation in units of the float32 numpy deviation (bound 4), per cols 8 / 255 / 256 / 1024 / 2048:
  k_rmsnorm 0.84 / 1.00 / 1.00 / 0.94 / 0.75, k_rmsnorm_hold 1.00 / 1.00 / 1.00 / 0.79 / 1.00. No kernel missed a check."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import frame_seam_cases as C
from frame_seam_cases import F32, GUARD, MF

pytestmark = pytest.mark.gpu

WORST = {}


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("H,B,V,k", C.FE_CASES)
def test_frame_embed(H, B, V, k):
    c = C.frame_embed_case(H, B, V, k)
    codes = np.r_[np.full(GUARD, C.CODE_SENTINEL), c.codes.reshape(-1), np.full(GUARD, C.CODE_SENTINEL)].astype(np.uint32)
    out = C.sentinel_f32(B * H + 2 * GUARD)
    q.frame_embed_ex(c.codec_emb, c.cp_embs, c.tok, c.logits, codes, c.frame_idx, MF, c.text_rows, c.trail_base, c.trail_len, c.pad_row, out,
                     text_ready=c.text_ready, guard=GUARD)
    assert (codes[:GUARD] == C.CODE_SENTINEL).all() and (codes[-GUARD:] == C.CODE_SENTINEL).all(), "codes guards"
    assert (_bits(out[:GUARD]) == C.OUT_SENTINEL_BITS).all() and (_bits(out[-GUARD:]) == C.OUT_SENTINEL_BITS).all(), "out guards"
    got_codes = codes[GUARD:-GUARD].reshape(B, MF, 16)
    for b in range(B):
        diff = np.argwhere(got_codes[b] != c.want_codes[b])
        assert diff.size == 0, f"row {b} ({c.state[b]}, f = {c.frame_idx[b]}): codes differ at (frame, slot) {diff[:4].tolist()}, argmax expected {c.last[b]}"
    got = out[GUARD:-GUARD].reshape(B, H)
    for b in range(B):
        bad = np.flatnonzero(_bits(got[b]) != _bits(c.want_out[b]))
        assert bad.size == 0, f"row {b} ({c.state[b]}, f = {c.frame_idx[b]}): {bad.size} of {H} outputs differ, first at {bad[:4]}"


@pytest.mark.parametrize("name", [c[0] for c in C.CG_CASES])
def test_cp_gather(name):
    kw, (out, qkv_out, codes), (want, want_qkv, want_codes) = C.cp_gather_case(name)
    q.cp_gather_ex(out=out, qkv_out=qkv_out, codes=codes, **kw)
    bad = np.flatnonzero(_bits(out) != _bits(want))
    assert bad.size == 0, f"out differs at {bad[:6]} (guard {GUARD}, pitch {kw['ld_out']})"
    if want_qkv is not None:
        bad = np.flatnonzero(_bits(qkv_out) != _bits(want_qkv))
        assert bad.size == 0, f"qkv_out differs at {bad[:6]}"
    if want_codes is not None:
        bad = np.flatnonzero(codes != want_codes)
        assert bad.size == 0, f"codes differ at {bad[:6]}: {codes[bad[:6]]} for {want_codes[bad[:6]]}"


@pytest.mark.parametrize("hold", [False, True], ids=["k_rmsnorm", "k_rmsnorm_hold"])
@pytest.mark.parametrize("cols", C.RN_COLS)
def test_rmsnorm(cols, hold):
    x, w, ref64, ref32 = C.rmsnorm_case(cols)
    R, ldy = C.RN_ROWS, cols + 3
    y = C.sentinel_f32(C.RN_FRONT + R * ldy)
    body = y[C.RN_FRONT:].reshape(R, ldy)
    old = np.random.default_rng(cols).standard_normal((R, cols)).astype(F32)
    body[:, :cols] = old
    before = y.copy()
    fi = rdy = None
    if hold:
        fi = np.full(R, 3, np.int32); rdy = np.full(R, C.INT_MAX, np.int32)
        rdy[C.RN_HELD[0]] = 3; rdy[C.RN_HELD[1]] = 1                   # frame_idx == text_ready and frame_idx > text_ready
    q.rmsnorm_ex(x, w, y, R, cols, x_off=(C.RN_RPS - 1) * cols, ldx=C.RN_RPS * cols, y_front=C.RN_FRONT, ldy=ldy, eps=C.RN_EPS, frame_idx=fi, text_ready=rdy)
    live = [r for r in range(R) if not (hold and r in C.RN_HELD)]
    mask = np.zeros(y.shape, bool); m = mask[C.RN_FRONT:].reshape(R, ldy); m[live, :cols] = True
    assert (_bits(y)[~mask] == _bits(before)[~mask]).all(), "a held row, a pitch gap or the front guard changed"
    got = body[live, :cols]
    assert np.isfinite(got).all()
    d_ref = C.rn_dev(ref32[live], ref64[live]); dev = C.rn_dev(got, ref64[live])
    key = ("k_rmsnorm_hold" if hold else "k_rmsnorm", cols)
    WORST[key] = dev / d_ref
    print(f"{key[0]} cols {cols}: dev {dev:.3e} = {dev / d_ref:.2f} x float32 numpy ({d_ref:.3e}); worst so far {max(WORST.values()):.2f}")
    assert dev <= 4 * d_ref, f"{key}: {dev:.3e} > 4 * {d_ref:.3e}"
