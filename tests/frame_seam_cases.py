"""Inputs and references of the op-level tests of the frame-seam kernels: k_frame_embed, k_cp_gather, k_rmsnorm / k_rmsnorm_hold
(through q3_frame_embed_ex, q3_cp_gather_ex, q3_rmsnorm_ex). numpy only.

k_frame_embed and k_cp_gather move table rows and add a fixed chain of float32 values: bf16 -> f32 is exact and every add is rounded
separately, so the references are bit-exact restatements (float32 numpy, left to right). The argmax is the first maximum, NaN never
wins, 0 when nothing compares. The norm is compared with float64; its bound is four times what the same formula in float32 numpy
deviates from float64 on the same inputs.

Row states of k_frame_embed (f = frame_idx, slot = min(f, max_frames - 1) is the code record it reads):
  live          f < max_frames, f < text_ready: records tok and the last code in slots 0 and 15 of frame f
  at_max        f == max_frames (a row frozen at the session's last frame): reads its last record, records nothing
  held          f >= text_ready: records nothing
  limit_frozen  a row k_sample froze at limit < max_frames. The kernel does not know the limit: to it the row is live, and it records
                into frame `limit` of the row's own block — one frame past the last one the row committed."""
from dataclasses import dataclass
from typing import Optional

import numpy as np

F32 = np.float32
INT_MAX = 2 ** 31 - 1
GUARD = 16
CODE_SENTINEL = np.uint32(0xDEADBEEF)
OUT_SENTINEL_BITS = np.uint32(0x7FC0BEEF)          # a NaN of known bits


def sentinel_f32(n):
    return np.full(n, OUT_SENTINEL_BITS, np.uint32).view(F32)


def bf16_bits(rng, shape, scale=1.0):
    """random bf16 values as uint16 bit patterns (truncated float32 normals)"""
    return ((scale * rng.standard_normal(shape)).astype(F32).view(np.uint32) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (bits.astype(np.uint32) << 16).view(F32)


def argmax_first(v):
    w = np.where(np.isnan(v), F32(-np.inf), v)
    return int(np.argmax(w))


def argmax_logits(rng, V, kind):
    """a logits row and its argmax. kind: "waves" = the maximum twice, low and high index in different waves; "lane" = twice in one
    thread's registers (indices 256 apart); "nan" = a NaN at a lower index than the maximum; "ninf" = all -inf (index 0)"""
    lg = rng.standard_normal(V).astype(F32)
    if kind == "ninf":
        return np.full(V, -np.inf, F32), 0
    if kind == "lane" and V > 256:
        lo = int(rng.integers(0, min(256, V - 256))); hi = lo + 256 * int(rng.integers(1, (V - 1 - lo) // 256 + 1))
    else:
        lo = int(rng.integers(0, max(1, min(V - 1, 40)))); hi = max(lo + 1, V - 1 - int(rng.integers(0, max(1, min(V // 4, 60)))))
        if V > 256 and (lo % 256) // 64 == (hi % 256) // 64:
            hi -= 64
    assert 0 <= lo < hi < V
    lg[[lo, hi]] = F32(10.0)
    if kind == "nan":
        lg[lo] = F32(np.nan)
        return lg, hi
    return lg, lo


# ------------------------------------------------------------------------------------------------------------------ k_frame_embed
# (H, B, cp_vocab, k): k rotates the row states and the argmax kinds, so the one- and three-row cases differ. cp_vocab 4100 does not
# fit the 16 registers per thread: block_argmax_first over memory
FE_CASES = ((8, 1, 5, 0), (8, 3, 4100, 0), (8, 3, 4100, 1), (8, 16, 4096, 0), (256, 3, 300, 3), (260, 16, 300, 1), (1024, 1, 300, 5), (260, 3, 2048, 6),
            (1024, 16, 5, 2), (256, 1, 2048, 4))
MF = 6
FE_STATES = (("live", 0), ("live", "tlen-1"), ("live", "tlen"), ("live", MF - 1), ("at_max", MF), ("held", 2), ("limit_frozen", 3), ("held", 4))
KINDS = ("waves", "lane", "nan", "ninf")


@dataclass
class FrameEmbedCase:
    H: int
    B: int
    V: int
    codec_emb: np.ndarray
    cp_embs: np.ndarray
    tok: np.ndarray
    logits: np.ndarray
    last: np.ndarray                 # expected argmax per row
    codes: np.ndarray                # [B][MF][16] before the launch
    frame_idx: np.ndarray
    text_rows: np.ndarray
    trail_base: np.ndarray
    trail_len: np.ndarray
    pad_row: np.ndarray
    text_ready: Optional[np.ndarray]
    state: list
    want_out: np.ndarray = None      # [B][H]
    want_codes: np.ndarray = None


_FE = {}


def frame_embed_case(H, B, V, k=0):
    key = (H, B, V, k)
    if key in _FE:
        return _FE[key]
    rng = np.random.default_rng(1000 * H + 10 * B + V + k)
    n_sem = 7
    tlen = np.array([(3, 1, 5)[b % 3] for b in range(B)], np.int32)
    state, fi, rdy = [], np.zeros(B, np.int32), np.full(B, INT_MAX, np.int32)
    for b in range(B):
        name, f = FE_STATES[(b + k) % len(FE_STATES)]
        f = int(tlen[b]) - 1 if f == "tlen-1" else int(tlen[b]) if f == "tlen" else f
        state.append(name); fi[b] = f
        if name == "held":
            rdy[b] = f - (b % 2)                       # f == text_ready and f > text_ready
    rows = [argmax_logits(rng, V, KINDS[(b + k) % 4]) for b in range(B)]
    c = FrameEmbedCase(H, B, V, bf16_bits(rng, (n_sem, H)), bf16_bits(rng, (15, V, H)), rng.integers(0, n_sem, B).astype(np.uint32),
                       np.stack([r[0] for r in rows]), np.array([r[1] for r in rows]), rng.integers(0, V, (B, MF, 16)).astype(np.uint32), fi,
                       rng.standard_normal((B * 8 + 2, H)).astype(F32), (np.arange(B) * 8).astype(np.int32), tlen,
                       (B * 8 + np.arange(B) % 2).astype(np.int32), None if B == 1 and "held" not in state else rdy, state)
    c.want_out = np.zeros((B, H), F32); c.want_codes = c.codes.copy()
    for b in range(B):
        f = int(fi[b]); slot = min(f, MF - 1)
        code = c.codes[b, slot].copy(); code[0] = c.tok[b]; code[15] = c.last[b]
        acc = bf16_to_f32(c.cp_embs[0, code[1]])
        for g in range(1, 15):
            acc = (acc + bf16_to_f32(c.cp_embs[g, code[1 + g]])).astype(F32)
        text = c.text_rows[c.trail_base[b] + f if f < tlen[b] else c.pad_row[b]]
        c.want_out[b] = ((bf16_to_f32(c.codec_emb[c.tok[b]]) + acc).astype(F32) + text).astype(F32)
        if f < MF and f < rdy[b]:
            c.want_codes[b, f, 0] = c.tok[b]; c.want_codes[b, f, 15] = c.last[b]
    _FE[key] = c
    return c


# ------------------------------------------------------------------------------------------------------------------ k_cp_gather
# (name, pass, source, qkv_dim): H and proj_dim are no multiples of 1024 (four workgroups share a row), out pitches are twice the row
CG_H, CG_PROJ, CG_B, CG_SEM, CG_V = 1500, 1028, 4, 9, 300
CG_CASES = (("pass0", 0, "hidden", 0), ("pass1_emb", 1, "emb", 0), ("pass1_proj", 1, "proj", 0), ("pass1_emb_qkv4", 1, "emb", 4),
            ("pass1_proj_qkv1540", 1, "proj", 1540), ("pass2_emb", 2, "emb", 0), ("pass2_proj_qkv4", 2, "proj", 4), ("pass7_emb_qkv1540", 7, "emb", 1540),
            ("pass15_proj", 15, "proj", 0))
CG_FRAMES = np.array([0, MF - 1, MF, 2], np.int32)          # row 2 sits at max_frames: its code is not recorded


def cp_gather_case(name):
    _, p, source, qkv_dim = [c for c in CG_CASES if c[0] == name][0]
    rng = np.random.default_rng(50 + p + qkv_dim)
    B, H = CG_B, CG_H
    n_rows = CG_SEM if p == 1 else CG_V
    width = CG_PROJ if source == "proj" else H
    kw = dict(pass_=p, B=B, H=H, ld_out=2 * width, guard=GUARD)
    out = sentinel_f32(B * 2 * width + 2 * GUARD)
    want = out.copy(); body = want[GUARD:-GUARD].reshape(B, 2 * width)
    rows = None
    codes = want_codes = None
    if p == 0:
        kw["last_hidden"] = rng.standard_normal((B, H)).astype(F32)
        body[:, :H] = kw["last_hidden"]
    else:
        if p == 1:
            kw["tok"] = rows = rng.integers(0, n_rows, B).astype(np.uint32)
        else:
            lg = [argmax_logits(rng, CG_V, KINDS[b % 4]) for b in range(B)]
            kw["cp_logits"] = np.stack([r[0] for r in lg]); rows = np.array([r[1] for r in lg])
            kw["frame_idx"] = CG_FRAMES; kw["max_frames"] = MF
            codes = np.full(B * MF * 16 + 2 * GUARD, CODE_SENTINEL, np.uint32)
            codes[GUARD:-GUARD] = rng.integers(0, CG_V, B * MF * 16)
            want_codes = codes.copy(); wc = want_codes[GUARD:-GUARD].reshape(B, MF, 16)
            for b in range(B):
                if CG_FRAMES[b] < MF:
                    wc[b, CG_FRAMES[b], p - 1] = rows[b]
        if source == "proj":
            kw["proj_tab"] = rng.standard_normal((n_rows, CG_PROJ)).astype(F32)
            body[:, :width] = kw["proj_tab"][rows]
        else:
            tab = bf16_bits(rng, (n_rows, H))
            kw["codec_emb" if p == 1 else "cp_emb"] = tab
            body[:, :H] = bf16_to_f32(tab[rows])
    qkv_out = want_qkv = None
    if qkv_dim:
        kw["qkv_tab"] = rng.standard_normal((n_rows, qkv_dim)).astype(F32); kw["ld_qkv_out"] = 2 * qkv_dim
        qkv_out = sentinel_f32(B * 2 * qkv_dim + 2 * GUARD); want_qkv = qkv_out.copy()
        want_qkv[GUARD:-GUARD].reshape(B, 2 * qkv_dim)[:, :qkv_dim] = kw["qkv_tab"][rows]
    return kw, (out, qkv_out, codes), (want, want_qkv, want_codes)


# ------------------------------------------------------------------------------------------------------------------ k_rmsnorm
RN_COLS = (8, 255, 256, 1024, 2048)
RN_ROWS, RN_RPS, RN_FRONT, RN_EPS = 5, 3, 7, 1e-6
RN_HELD = (1, 3)


def rmsnorm_case(cols):
    """x [rows][rows_per_seq][cols], the launch norms each sequence's LAST row (offset (rps - 1) * cols, pitch rps * cols, as the talker's
    final norm of a multi-row step); y rows have a pitch of cols + 3 behind a front guard. Returns x, w, the float64 and float32 results"""
    rng = np.random.default_rng(70 + cols)
    x = (rng.standard_normal((RN_ROWS, RN_RPS, cols)) * rng.uniform(0.05, 20.0, (RN_ROWS, 1, 1))).astype(F32)
    w = (1.0 + 0.2 * rng.standard_normal(cols)).astype(F32)
    xl = x[:, -1, :]
    x64 = xl.astype(np.float64)
    ref64 = x64 / np.sqrt((x64 * x64).mean(axis=1, keepdims=True) + RN_EPS) * w.astype(np.float64)
    ref32 = (xl / np.sqrt((xl * xl).mean(axis=1, keepdims=True, dtype=F32) + F32(RN_EPS)) * w).astype(F32)
    return x, w, ref64, ref32


def rn_dev(a, ref64):
    """largest deviation of a row set from float64, relative to each row's largest magnitude"""
    return float(np.max(np.max(np.abs(a.astype(np.float64) - ref64), axis=1) / np.max(np.abs(ref64), axis=1)))
