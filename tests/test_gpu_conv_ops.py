"""Op-level tests of the vocoder conv family (q3_kernels_codec.hip): every kernel instance launch_conv1d / launch_transconv1d_taps /
launch_resunit can pick under the default dispatch, driven one launch at a time through q3_conv_ex and compared with float64 numpy
of the definition; plus launch_layernorm_c / launch_rmsnorm_c (q3_norm_c) and launch_dwconv7 (q3_dwconv7).

One shape table (CASES): each row names the ConvPath code it is chosen against. test_table_reaches_the_paths_it_names walks it through
q3_conv_path / q3_resunit_path — the launchers' own decision function — without a GPU; the GPU cases additionally assert the code
q3_conv_ex reports for the launch it made.

Checks per case:
  * dense: seeded normal x, w ~ N(0, 1 / (cin k)), snake alpha / beta in +-0.5; float64 reference of the definition (causal conv with
    left zero padding; transposed conv as scatter-add over [cin][cout][k] trimmed to L stride; the residual unit as
    y + conv1x1(snake(conv7(x) + b1)) + b2); rel_err < 2e-5, the project's figure for f32 accumulation over K <= 6144 (every reduction
    here is cin k <= 5376). A subset also runs the CPU oracle (q3o_causal_conv1d, q3o_causal_trans_conv1d, q3o_snake_beta) and requires
    the same bound of it: the bound is the arithmetic's, not the kernel's;
  * two-plane mode (planes = 2, k in {1, 2, 7}): float64 of the mode itself, sum (wh + wm)(xh + xm) - wm xm with h = bf16_rne(v),
    m = bf16_rne(v - h) computed here, same 2e-5 (only accumulation error remains); the distance to the true result is recorded only;
  * exact: integer inputs for which every product and every partial sum in any order is an integer below 2^24 — bit equality;
  * nothing else written: sentinels in a 64-float guard in front of and behind y and y2;
  * same bits across kernels that promise it (k_lin_small vs the tiled kernel, the fused unit vs its two launches, L vs L + 128).

The 192-channel fused residual unit is behind Q3_CODEC_UNIT_FUSE_192 and off by default: not tested here (C = 192 is a refusal case).
Measured errors go to conv_ops.json in the report directory of the GPU tests (_dump of test_gpu_parity.py; worst per path: DESIGN.md)."""
import collections
import math
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from common import rel_err
from test_gpu_parity import _dump          # the report directory of the GPU tests

gpu = pytest.mark.gpu

# the shapes below are chosen against the DEFAULT dispatch; these knobs are read once per process and would silently move a case
KNOBS = ["Q3_CONV_F32", "Q3_CONV_VALU", "Q3_CONV_TM4", "Q3_CONV_PW1_GEO", "Q3_CONV_CIS32", "Q3_CONV_NO_SMALL", "Q3_CONV_NO_SMALL_TILES",
         "Q3_CODEC_NO_UNIT_FUSE", "Q3_CODEC_UNIT_FUSE_192", "Q3_NORM_C_OLD"]
assert [k for k in KNOBS if k in os.environ] == [], "dispatch knobs set: the shape table would not reach the kernels it names"

TOL = 2e-5
SENT = np.float32(-7.0625e33)            # no kernel computes this value
GUARD = 64
RESULTS = collections.OrderedDict()
GPU_RAN = []

# ConvPath codes (include/q3tts.h): kernel in the low five bits, then flags
OUT1, OUT1_V4, SMALL4, SMALL8, G96_TM4, G4W128, G4W256, G64x128, G64x64, G128x128, G96_6W, MFMA64, MFMA32, VALU, UNIT3, UNIT6 = range(1, 17)
PRE, SEG, CIS128, NP2 = 32, 64, 128, 256
CONV, TCONV, UNIT = 0, 1, 2

Case = collections.namedtuple("Case", "path kind cout cin L k dil stride packed resid planes opts")


def C(path, cout, cin, L, k, dil=1, *, kind=CONV, stride=1, packed=True, resid=False, planes=3, **opts):
    """opts: bias (default True), y2, snake (on load), post (on the output), scale, inplace (the residual is y itself), act, oracle (CPU oracle too)"""
    return Case(path, kind, cout, cin, L, k, dil, stride, packed, resid or opts.get("inplace", False), planes, opts)


CASES = []
# k_lin_small_bf16x3<4>: k = 1, cin % 512 == 0, cin < 1024, L <= 32, cout % 64 == 0
CASES += [C(SMALL4 | SEG, 64, 512, L, 1, bias=(L != 10), snake=(L == 10)) for L in (1, 10, 32)]
# k_lin_small_bf16x3<8>: cin >= 1024; L > 32 stays here while (cout / 32) * ceil(L / 32) <= 512 ("small tiles")
CASES += [C(SMALL8 | SEG, 64, cin, L, 1, inplace=(L == 33), scale=(L == 33), post=(L == 100), y2=(L == 100 and cin == 1536))
          for cin in (1024, 1536, 4096) for L in (31, 32, 33, 100)]
# 96 co x 128 t, three waves, T_M = 4: taps, cout in {96, 192}, L >= 4096. 4096: 32 time tiles; 4097 / 4173: 33 (the nt & ~7 tail, one column /
# 77 columns in the last tile). cin 48: a 16-channel last stage; dilation 9: halo 54
CASES += [C(G96_TM4, cout, cin, L, k, dil, bias=(L != 4097), post=(L == 4173), y2=(L == 4173 and k == 7), snake=(L == 4096 and k == 2))
          for (k, dil, cin) in ((2, 1, 48), (7, 9, 32)) for cout in (96, 192) for L in (4096, 4097, 4096 + 77)]
# four waves x 32 co x 128 t: taps, cout % 128 == 0, L >= 4096, big_tiles = ceil(L / 128) * (cout / 128) * phases >= 192.
# cout 128: 24449 = 191 * 128 + 1 is the first L on the line (192 tiles, L % 128 == 1); cout 256: 12161 = 95 * 128 + 1; 12287: L % 128 == 127
CASES += [C(G4W128, 128, 16, 24449, 2), C(G4W128, 128, 48, 24577, 7, 3, post=True, y2=True), C(G4W128, 256, 32, 12161, 7, bias=False),
          C(G4W128, 256, 16, 12287, 2, snake=True), C(G4W128, 128, 16, 24576, 7)]
# tails of the XCD tile order longer than one tile in the large geometries (a one-tile tail cannot show a shifted tail mapping):
# 36 = 32 + 4 time tiles, 196 = 192 + 4, 99 = 96 + 3, 197 = 192 + 5, 1027 = 1024 + 3, 26 = 24 + 2
CASES += [C(G96_TM4, 192, 48, 4096 + 3 * 128 + 5, 7, 3), C(G4W128, 128, 16, 24449 + 4 * 128, 2), C(G4W128, 256, 32, 12161 + 3 * 128, 7, bias=False),
          C(G64x128 | PRE, 128, 16, 24449 + 5 * 128, 1, resid=True), C(G128x128, 128, 16, 130945 + 3 * 128, 1, bias=False),
          C(G128x128, 1024, 16, 2945 + 2 * 128, 2)]
# one tile below the line the same layer takes the 64 x 64 tiles (382 of them: tile count % 8 == 6)
CASES += [C(G64x64, 128, 16, 24448, 7)]
# 64 co x 128 t with the batched residual loads (PRE): k = 1 with a residual, cout % 64 == 0 and != 96, big_tiles >= 192
CASES += [C(G64x128 | PRE, 128, 48, 24449, 1, inplace=True, post=True, y2=True), C(G64x128 | PRE, 192, 32, 24449 + 77, 1, resid=True, scale=True),
          C(G64x128 | PRE | SEG, 128, 512, 24449, 1, inplace=True, bias=False)]
# 64 co x 64 t with 128-channel stages: k = 1, no residual, cout % 128 == 0, 192 <= big_tiles < 1024, cin >= 256.
# cin 320: a 64-channel last stage (n16 = 4, neither 2 nor 8); cin 512: segmented summation
CASES += [C(G64x64 | CIS128, 1024, 256, 2945, 1, act=1), C(G64x64 | CIS128, 128, 320, 24449 + 77, 1, snake=True),
          C(G64x64 | CIS128 | SEG, 256, 512, 12161, 1, bias=False), C(G64x64, 128, 48, 24449, 1), C(G64x64, 256, 240, 12161, 1)]
# 128 co x 128 t: k = 1 without a residual at big_tiles >= 1024 (130945 = 1023 * 128 + 1); taps below L = 4096 at big_tiles >= 192
CASES += [C(G128x128, 128, 16, 130945, 1), C(G128x128, 128, 48, 130945 + 50, 1, bias=False), C(G128x128 | SEG, 128, 512, 130945, 1),
          C(G128x128, 1024, 16, 2945, 7), C(G128x128, 768, 48, 4000, 3),
          C(G128x128, 768, 16, 512, 16, kind=TCONV, stride=8, post=True, y2=True)]
# 96 co x 128 t, six waves: cout in {96, 192} below L = 4096. L 5 < halo; 300: 3 time tiles; 1100: 9 (nt > 8, nt % 8 == 1)
CASES += [C(G96_6W, 96, 16, 5, 7, 9), C(G96_6W, 192, 48, 300, 7, 3, post=True, y2=True), C(G96_6W, 96, 32, 1100, 7, 1, snake=True, oracle=True),
          C(G96_6W, 192, 16, 1100, 2, 1, bias=False), C(G96_6W, 96, 48, 100, 2, 1), C(G96_6W, 192, 64, 1, 7, 1), C(G96_6W, 96, 16, 77, 5, 9),
          C(G96_6W | PRE, 96, 96, 300, 1, inplace=True, post=True, y2=True), C(G96_6W | PRE, 192, 48, 1100, 1, resid=True, scale=True),
          C(G96_6W, 96, 16, 4097, 1), C(G96_6W | SEG, 192, 512, 300, 1), C(G96_6W | PRE | SEG, 96, 512, 129, 1, inplace=True)]
# 64 co x 64 t: cout % 64 == 0 on small grids; 128-channel stages from cin 256 on
# (cin 304 / 272: a 48- / 16-channel last stage under CIS = 128, n16 = 3 / 1)
CASES += [C(G64x64, 64, 16, 7, 7), C(G64x64, 320, 48, 100, 3, 2, oracle=True), C(G64x64 | CIS128, 64, 320, 65, 1, post=True),
          C(G64x64 | CIS128, 64, 304, 65, 1), C(G64x64 | CIS128, 128, 272, 70, 1, bias=False),
          C(G64x64 | CIS128 | PRE, 320, 256, 600, 1, inplace=True), C(G64x64 | PRE, 64, 80, 33, 1, resid=True, scale=True),
          C(G64x64 | CIS128 | SEG, 64, 512, 33, 1), C(G64x64 | CIS128 | SEG | PRE, 64, 512, 600, 1, resid=True), C(G64x64, 64, 32, 1100, 5, 1, bias=False),
          C(G64x64, 128, 16, 24448, 2)]
# activations share conv_act: one small geometry each
CASES += [C(G64x64, 64, 32, 100, 3, act=1), C(G96_6W, 96, 32, 100, 7, act=3), C(G64x64 | CIS128, 64, 256, 70, 1, act=4),
          C(MFMA64, 64, 24, 100, 3, packed=False, act=5), C(VALU, 8, 16, 100, 5, packed=False, act=6), C(SMALL4 | SEG, 64, 512, 20, 1, act=1)]
# fallbacks. Packed weights without a geometry (cout 160, 32) and unpacked weights: the f32-MFMA kernel (64-channel tiles when cout % 64 == 0);
# k = 5 unpacked and cout < 32: the VALU kernel
CASES += [C(MFMA32, 160, 16, 300, 7, 3), C(MFMA32, 32, 48, 5, 1), C(MFMA64, 64, 1, 130, 1, packed=False), C(MFMA64, 128, 24, 257, 2, packed=False, snake=True, oracle=True),
          C(MFMA32, 40, 80, 300, 3, 9, packed=False, post=True, y2=True), C(MFMA32, 96, 24, 1100, 7, 9, packed=False, inplace=True, scale=True),
          C(MFMA64, 64, 80, 5, 7, 9, packed=False, bias=False), C(VALU, 64, 24, 200, 5, 2, packed=False, oracle=True), C(VALU, 8, 80, 129, 7, 9, packed=False, snake=True),
          C(VALU, 24, 1, 5, 3, packed=False, resid=True, scale=True, post=True, y2=True), C(VALU, 32, 16, 300, 5, bias=False)]
# cout = 1: the float4 form needs k = 7, dilation 1, L % 4 == 0; clamp (act 2)
CASES += [C(OUT1_V4, 1, 96, 1920, 7, act=2, snake=True, packed=False), C(OUT1_V4, 1, 24, 4, 7, act=2, packed=False),
          C(OUT1, 1, 96, 1921, 7, act=2, snake=True, packed=False), C(OUT1, 1, 16, 300, 3, act=2, packed=False),
          C(OUT1, 1, 16, 300, 7, 2, act=2, bias=False, packed=False)]
# transposed convs: k = stride * taps; two taps (the decoder blocks) at strides 2, 3, 4, 5, 8; one tap (the upsample stages) at stride 2
CASES += [C(G64x64, 64, 32, 100, 4, kind=TCONV, stride=2, oracle=True), C(G96_6W, 96, 48, 77, 6, kind=TCONV, stride=3, post=True, y2=True),
          C(G64x64, 64, 16, 130, 8, kind=TCONV, stride=4, bias=False), C(G96_6W, 192, 32, 300, 10, kind=TCONV, stride=5, snake=True),
          C(G4W128, 128, 16, 4096 + 77, 16, kind=TCONV, stride=8, post=True, y2=True), C(G96_TM4, 96, 48, 4097, 6, kind=TCONV, stride=3),
          C(G64x64 | CIS128, 64, 256, 65, 2, kind=TCONV, stride=2), C(G64x64 | CIS128 | SEG, 128, 512, 33, 2, kind=TCONV, stride=2, oracle=True),
          C(G64x64, 768, 16, 4096, 2, kind=TCONV, stride=2), C(MFMA64, 64, 24, 100, 4, kind=TCONV, stride=2, packed=False, oracle=True),
          C(MFMA32, 40, 16, 77, 10, kind=TCONV, stride=5, packed=False, post=True), C(VALU, 8, 16, 130, 8, kind=TCONV, stride=4, packed=False)]
# the fused residual unit: C = 96, L >= 4096, dilation 1 / 3 / 9
CASES += [C(UNIT3 | (NP2 if planes == 2 else 0), 96, 96, L, 7, dil, kind=UNIT, planes=planes, y2=(dil != 3), post=(dil != 3))
          for L in (4096, 4096 + 77) for dil in (1, 3, 9) for planes in (3, 2)]
# two-plane mode, k in {1, 2, 7}: one case per kernel that has two-plane instances
CASES += [C(SMALL4 | SEG | NP2, 64, 512, 10, 1, planes=2), C(SMALL8 | SEG | NP2, 64, 1024, 33, 1, planes=2), C(G96_TM4 | NP2, 96, 48, 4097, 7, 3, planes=2),
          C(G4W128 | NP2, 128, 16, 24449, 2, planes=2), C(G64x128 | PRE | NP2, 128, 48, 24449, 1, planes=2, inplace=True),
          C(G64x64 | CIS128 | NP2, 128, 320, 24449 + 77, 1, planes=2), C(G128x128 | NP2, 1024, 16, 2945, 7, planes=2),
          C(G96_6W | NP2, 192, 48, 300, 7, 3, planes=2), C(G64x64 | NP2, 64, 16, 130, 8, kind=TCONV, stride=4, planes=2)]
REFUSALS = [dict(L=4095), dict(C=192), dict(dil=2), dict(y2_is_x=True), dict(packed=False)]

# the same table by id; rows with the same parameters are written once
CASES = list(collections.OrderedDict((c[:-1] + (tuple(sorted(c.opts.items())),), c) for c in CASES).values())


def _id(c):
    o = "".join(f"-{k}" if v is True else f"-{k}{v}" for k, v in sorted(c.opts.items()) if v not in (False, None))
    return f"{('conv', 'tconv', 'unit')[c.kind]}-p{c.path}-co{c.cout}-ci{c.cin}-L{c.L}-k{c.k}-d{c.dil}-s{c.stride}-{'pk' if c.packed else 'f32'}-np{c.planes}{o}"


IDS = [_id(c) for c in CASES]
assert len(set(IDS)) == len(IDS)


def _table_path(c):
    if c.kind == UNIT:
        return q.resunit_path(c.cout, c.L, c.dil, c.packed, False, c.planes)
    if c.kind == TCONV:
        return q.conv_path(c.cout, c.cin, c.L, c.k // c.stride, 1, c.stride, c.packed, False, c.planes, False)
    return q.conv_path(c.cout, c.cin, c.L, c.k, c.dil, 1, c.packed, c.resid, c.planes, True)


# ---------------------------------------------------------------- the table against the dispatcher (no GPU)
def test_table_reaches_the_paths_it_names():
    for c in CASES:
        got = _table_path(c)
        assert got == c.path, f"{_id(c)}: dispatches to {q.conv_path_name(got)} ({got}), the table names {q.conv_path_name(c.path)}"
    assert q.conv_path_name(G64x64 | CIS128 | SEG) == "k_conv_bf16x3<64co x 64t> SEG CIS=128" and q.conv_path_name(1 << 20) == "invalid"
    assert q.resunit_path(96, 4095, 1) == 0 and q.resunit_path(192, 4096, 1) == 0 and q.resunit_path(96, 4096, 2) == 0
    assert q.resunit_path(96, 4096, 1, ya_is_xa=True) == 0 and q.resunit_path(96, 4096, 1, packed=False) == 0
    # launch_conv1d's own refusals: more than 7 taps, a halo beyond 54, no columns
    assert q.conv_path(64, 16, 100, 8) == 0 and q.conv_path(64, 16, 100, 7, 10) == 0 and q.conv_path(64, 16, 0, 1) == 0


def test_table_covers_every_path_of_the_default_dispatch():
    """Every code the dispatcher returns over a grid of shapes around each of its thresholds is in the table — with the two-plane flag
    masked off for the grid (the table runs two planes once per kernel that has such instances, asserted separately)."""
    seen = set()
    for cout in (1, 8, 32, 40, 64, 96, 128, 160, 192, 256, 320, 768, 1024, 4096):
        for cin in (1, 16, 24, 48, 80, 256, 320, 512, 1024, 4096):
            for L in (1, 32, 33, 100, 600, 2945, 4095, 4096, 4097, 12161, 24448, 24449, 130944, 130945):
                for k in (1, 2, 3, 5, 7):
                    for phases in (1, 2, 8):
                        for packed in (0, 1):
                            for resid in ((0, 1) if phases == 1 else (0,)):
                                for al in ((0, 1) if cout == 1 else (1,)):
                                    seen.add(_lib.lib.q3_conv_path(cout, cin, L, k, 1, phases, packed, resid, 3, al))
    for Cc in (96, 192):
        for L in (4095, 4096):
            seen.add(q.resunit_path(Cc, L, 1))
    seen.discard(0)
    table = {c.path & ~NP2 for c in CASES}
    missing = sorted(seen - table)
    assert missing == [], "paths of the default dispatch without a table row: " + ", ".join(f"{m} = {q.conv_path_name(m)}" for m in missing)
    # the instances only a knob reaches are not in the table; everything else is
    assert {c.path & 31 for c in CASES} == set(range(1, 17)) - {G4W256, UNIT6}
    two = {c.path & 31 for c in CASES if c.path & NP2}
    assert two == {SMALL4, SMALL8, G96_TM4, G4W128, G64x128, G64x64, G128x128, G96_6W, UNIT3}


# The conv launches of a whole-utterance decode at the production decoder shape (the weights q3_model_finalize packs, at the lengths of T
# frames): (name, kind, cout, cin, L / T, k, dilation, phases, residual). The codes below were produced by the dispatch rules as they stood
# BEFORE kernel selection was split from the launch (transcribed by hand into a script and run over this list): the split must not move
# any production shape to another kernel.
def _production_rows(T):
    CD, Q, LAT, DH, QD, DI, DIM = 256, 512, 1024, 512, 1024, 1024, 1536
    rows = [("first_proj", CONV, Q, CD, T, 1, 1, 1, False), ("rest_proj", CONV, Q, CD, T, 1, 1, 1, True), ("pre_conv", CONV, LAT, Q, T, 3, 1, 1, False),
            ("input_proj", CONV, DH, LAT, T, 1, 1, 1, False), ("q", CONV, QD, DH, T, 1, 1, 1, False), ("qkv", CONV, 3 * QD, DH, T, 1, 1, 1, False),
            ("o", CONV, DH, QD, T, 1, 1, 1, True), ("gate", CONV, DI, DH, T, 1, 1, 1, False), ("gate_up", CONV, 2 * DI, DH, T, 1, 1, 1, False),
            ("down", CONV, DH, DI, T, 1, 1, 1, True), ("output_proj", CONV, LAT, DH, T, 1, 1, 1, False)]
    L = T
    for i, r in enumerate((2, 2)):
        rows.append((f"up{i}.transconv", TCONV, LAT, LAT, L, 1, 1, r, False))
        L *= r
        rows += [(f"up{i}.pw1", CONV, 4 * LAT, LAT, L, 1, 1, 1, False), (f"up{i}.pw2", CONV, LAT, 4 * LAT, L, 1, 1, 1, True)]
    rows.append(("decoder.0", CONV, DIM, LAT, L, 7, 1, 1, False))
    Cc = DIM
    for b, rate in enumerate((8, 5, 4, 3)):
        rows.append((f"blk{b}.transconv", TCONV, Cc // 2, Cc, L, 2, 1, rate, False))
        L *= rate; Cc //= 2
        for d in (1, 3, 9):
            rows += [(f"blk{b}.unit_d{d}", UNIT, Cc, Cc, L, 7, d, 1, False), (f"blk{b}.conv7_d{d}", CONV, Cc, Cc, L, 7, d, 1, False)]
        rows.append((f"blk{b}.conv1", CONV, Cc, Cc, L, 1, 1, 1, True))
    rows.append(("final", CONV, 1, Cc, L, 7, 1, 1, False))
    return rows


PRODUCTION_CODES = {
    # (planes, T): one code per row of _production_rows(T)
    (3, 10): [137, 169, 9, 68, 67, 67, 68, 67, 67, 68, 67, 201, 68, 68, 201, 68, 68, 9, 9, 0, 9, 0, 9, 0, 9, 169, 9, 0, 9, 0, 9, 0, 9, 169, 11, 0, 5, 0, 5, 0, 5, 43, 5, 15, 5, 15, 5, 15, 5, 43, 2],
    (3, 11): [137, 169, 9, 68, 67, 67, 68, 67, 67, 68, 67, 201, 68, 68, 201, 68, 68, 9, 9, 0, 9, 0, 9, 0, 9, 169, 9, 0, 9, 0, 9, 0, 9, 169, 11, 0, 5, 0, 5, 0, 5, 43, 5, 15, 5, 15, 5, 15, 5, 43, 2],
    (3, 128): [137, 169, 9, 68, 201, 201, 68, 201, 201, 68, 201, 201, 201, 68, 201, 201, 68, 9, 10, 0, 6, 0, 6, 0, 6, 40, 6, 0, 6, 0, 6, 0, 6, 40, 5, 0, 5, 0, 5, 0, 5, 40, 5, 15, 5, 15, 5, 15, 5, 43, 2],
    (3, 640): [137, 169, 9, 68, 201, 201, 68, 201, 201, 68, 201, 201, 201, 233, 201, 201, 233, 10, 10, 0, 6, 0, 6, 0, 6, 40, 6, 0, 6, 0, 6, 0, 6, 40, 5, 0, 5, 0, 5, 0, 5, 40, 5, 15, 5, 15, 5, 15, 5, 43, 2],
    (2, 10): [393, 425, 9, 324, 323, 323, 324, 323, 323, 324, 323, 457, 324, 324, 457, 324, 324, 265, 265, 0, 265, 0, 265, 0, 265, 425, 265, 0, 265, 0, 265, 0, 265, 425, 267, 0, 261, 0, 261, 0, 261, 299, 261, 271, 261, 271, 261, 271, 261, 299, 2],
    (2, 11): [393, 425, 9, 324, 323, 323, 324, 323, 323, 324, 323, 457, 324, 324, 457, 324, 324, 265, 265, 0, 265, 0, 265, 0, 265, 425, 265, 0, 265, 0, 265, 0, 265, 425, 267, 0, 261, 0, 261, 0, 261, 299, 261, 271, 261, 271, 261, 271, 261, 299, 2],
    (2, 128): [393, 425, 9, 324, 457, 457, 324, 457, 457, 324, 457, 457, 457, 324, 457, 457, 324, 265, 266, 0, 262, 0, 262, 0, 262, 296, 262, 0, 262, 0, 262, 0, 262, 296, 261, 0, 261, 0, 261, 0, 261, 296, 261, 271, 261, 271, 261, 271, 261, 299, 2],
    (2, 640): [393, 425, 9, 324, 457, 457, 324, 457, 457, 324, 457, 457, 457, 489, 457, 457, 489, 266, 266, 0, 262, 0, 262, 0, 262, 296, 262, 0, 262, 0, 262, 0, 262, 296, 261, 0, 261, 0, 261, 0, 261, 296, 261, 271, 261, 271, 261, 271, 261, 299, 2],
}


def test_production_shapes_keep_their_kernels():
    assert sorted(PRODUCTION_CODES) == sorted((p, T) for p in (2, 3) for T in (10, 11, 128, 640))
    for (planes, T), want in PRODUCTION_CODES.items():
        rows = _production_rows(T)
        assert len(rows) == len(want) == 51
        for (name, kind, cout, cin, L, k, dil, phases, resid), code in zip(rows, want):
            if kind == UNIT:
                got = q.resunit_path(cout, L, dil, True, False, planes)
            else:
                got = q.conv_path(cout, cin, L, k, dil, phases, True, resid, planes, True)
            assert got == code, f"T={T} planes={planes} {name}: {q.conv_path_name(got)} ({got}), was {q.conv_path_name(code)} ({code})"


# ---------------------------------------------------------------- float64 references of the definitions
def bf16_rne(v):
    """float32 array rounded to bf16 (round to nearest even), as float32"""
    u = np.ascontiguousarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(np.shape(v))


def conv_ref(x, w, dil):
    """causal conv, left zero padding: y[co][t] = sum_ci sum_kk w[co][ci][kk] x[ci][t - (k - 1 - kk) dil]; float64"""
    cout, cin, k = w.shape
    L = x.shape[1]
    y = np.zeros((cout, L))
    for kk in range(k):
        sh = (k - 1 - kk) * dil
        if sh < L:
            y[:, sh:] += np.ascontiguousarray(w[:, :, kk]) @ x[:, :L - sh]          # (a strided operand would bypass BLAS)
    return y


def tconv_ref(x, w, stride):
    """transposed conv as scatter-add over w [cin][cout][k]: full[co][j stride + kk] += w[ci][co][kk] x[ci][j], trimmed to L stride"""
    cin, cout, k = w.shape
    L = x.shape[1]
    full = np.zeros((cout, (L - 1) * stride + k))
    for kk in range(k):
        full[:, kk:kk + (L - 1) * stride + 1:stride] += np.ascontiguousarray(w[:, :, kk].T) @ x
    return full[:, :L * stride]


def snake_ref(x, alpha, beta):
    return x + np.sin(x * np.exp(alpha)[:, None]) ** 2 / (np.exp(beta)[:, None] + 1e-9)


_erf = np.frompyfunc(math.erf, 1, 1)


def act_ref(v, act):
    if act == 1:
        return 0.5 * v * (1.0 + _erf(v * math.sqrt(0.5)).astype(np.float64))
    if act == 3:
        return np.maximum(v, 0.0)
    if act == 4:
        return np.tanh(np.maximum(v, 0.0))
    if act == 5:
        return 1.0 / (np.exp(-v) + 1.0)
    if act == 6:
        return np.where(v > 0, v, np.expm1(np.minimum(v, 0.0)))
    return v


def _buf(n, fill=None):
    """[64 sentinels][n floats][64 sentinels]"""
    b = np.full(n + 2 * GUARD, SENT, dtype=np.float32)
    if fill is not None:
        b[GUARD:GUARD + n] = fill.reshape(-1)
    return b


def _guards_ok(b, n, what):
    s = SENT.view(np.uint32)
    assert (b[:GUARD].view(np.uint32) == s).all(), f"{what}: written in front of the buffer"
    assert (b[GUARD + n:].view(np.uint32) == s).all(), f"{what}: written behind the result"


def _record(c, **figs):
    RESULTS.setdefault(_id(c), {"path": q.conv_path_name(c.path)}).update(figs)
    print(_id(c), q.conv_path_name(c.path), figs)


@pytest.fixture(scope="module", autouse=True)
def _dump_results():
    yield
    if GPU_RAN:
        worst = {}
        for r in RESULTS.values():
            for k, v in r.items():
                if k != "path" and isinstance(v, float):
                    worst.setdefault(r["path"], {})[k] = max(worst.get(r["path"], {}).get(k, 0.0), v)
        _dump("conv_ops.json", {"worst_per_path": worst, "cases": RESULTS})


def _inputs(c, seed=0):
    """seeded dense inputs of a case: x, w (layout of the kind), and the optional operands its opts ask for"""
    rng = np.random.default_rng([c.cout, c.cin, c.L, c.k, c.dil, c.stride, c.kind, seed])
    o = c.opts
    d = {}
    d["x"] = rng.standard_normal((c.cin, c.L)).astype(np.float32)
    shape = (c.cin, c.cout, c.k) if c.kind == TCONV else (c.cout, c.cin, c.k)
    taps = c.k // c.stride
    d["w"] = (rng.standard_normal(shape) / math.sqrt(c.cin * taps)).astype(np.float32)
    d["b"] = rng.standard_normal(c.cout).astype(np.float32) if o.get("bias", True) else None
    pair = lambda n: (rng.uniform(-0.5, 0.5, n).astype(np.float32), rng.uniform(-0.5, 0.5, n).astype(np.float32))
    d["snake"] = pair(c.cin) if o.get("snake") else None
    d["post"] = pair(c.cout) if o.get("post") else None
    d["scale"] = rng.uniform(0.5, 1.5, c.cout).astype(np.float32) if o.get("scale") else None
    d["resid"] = rng.standard_normal((c.cout, c.L * c.stride)).astype(np.float32) if c.resid else None
    if c.kind == UNIT:
        d["w2"] = (rng.standard_normal((c.cout, c.cin, 1)) / math.sqrt(c.cin)).astype(np.float32)
        d["b2"] = rng.standard_normal(c.cout).astype(np.float32)
        d["mid"] = pair(c.cout)
        d["resid"] = rng.standard_normal((c.cout, c.L)).astype(np.float32)
    return d


def _reference(c, d, two_plane=False):
    """float64 of the definition -> (raw, activated or None). two_plane: float64 of the mode, sum (wh + wm)(xh + xm) - wm xm"""
    f8 = lambda a: a.astype(np.float64)
    x = f8(d["x"])
    if d["snake"] is not None:
        x = snake_ref(x, f8(d["snake"][0]), f8(d["snake"][1]))

    def product(xv, wv, fn):
        if not two_plane:
            return fn(f8(xv), f8(wv))
        xv = np.asarray(xv, dtype=np.float32); wv = np.asarray(wv, dtype=np.float32)
        xh = bf16_rne(xv); xm = bf16_rne(xv - xh); wh = bf16_rne(wv); wm = bf16_rne(wv - wh)
        return fn(f8(xh) + f8(xm), f8(wh) + f8(wm)) - fn(f8(xm), f8(wm))
    if two_plane:
        assert d["snake"] is None          # the split is of the kernel's f32 snake value, which numpy does not reproduce to the bit
        x = d["x"]
    if c.kind == TCONV:
        v = product(x, d["w"], lambda a, b: tconv_ref(a, b, c.stride))
    else:
        v = product(x, d["w"], lambda a, b: conv_ref(a, b, c.dil))
    if d["b"] is not None:
        v = v + f8(d["b"])[:, None]
    if c.kind == UNIT:
        assert not two_plane
        mid = snake_ref(v, f8(d["mid"][0]), f8(d["mid"][1]))
        v = f8(d["resid"]) + (conv_ref(mid, f8(d["w2"]), 1) + f8(d["b2"])[:, None])
    else:
        v = act_ref(v, c.opts.get("act", 0))
        if d["scale"] is not None:
            v = v * f8(d["scale"])[:, None]
        if d["resid"] is not None:
            v = f8(d["resid"]) + v
        if c.opts.get("act", 0) == 2:
            v = np.clip(v, -1.0, 1.0)
    va = snake_ref(v, f8(d["post"][0]), f8(d["post"][1])) if d["post"] is not None else None
    return v, va


def _tables(pr):
    """(alpha, beta) -> the (a, 1 / b) tables of launch_snake_tables, in float32 as the engine holds them"""
    return None if pr is None else (np.exp(pr[0].astype(np.float64)).astype(np.float32), (1.0 / (np.exp(pr[1].astype(np.float64)) + 1e-9)).astype(np.float32))


def _run(c, d, what, raw_tables=True, planes=None):
    """one q3_conv_ex launch of the case; asserts the reported path and the guards -> (y, y2) as [cout][L stride]"""
    n = c.cout * c.L * c.stride
    inplace = c.opts.get("inplace", False) or c.kind == UNIT
    y = _buf(n, d["resid"] if inplace else None)
    y2 = _buf(n) if c.opts.get("y2") else None
    conv = (lambda p: p) if raw_tables else _tables
    kw = dict(dil=c.dil, stride=c.stride, b=d["b"], snake=conv(d["snake"]), post=conv(d["post"]), scale=d["scale"], act=c.opts.get("act", 0),
              planes=c.planes if planes is None else planes, packed=c.packed, snake_raw=raw_tables, y=y, y2=y2, y_front=GUARD)
    if c.kind == UNIT:
        kw.update(w2=d["w2"], b2=d["b2"], mid=conv(d["mid"]))
    elif inplace:
        kw["resid_in_place"] = True
    elif d["resid"] is not None:
        kw["resid"] = d["resid"]
    _, _, path = q.conv_ex(c.kind, d["x"], d["w"], **kw)
    GPU_RAN.append(1)
    if planes is None:
        assert path == c.path, f"{what}: ran {q.conv_path_name(path)} ({path}), the table names {q.conv_path_name(c.path)}"
    _guards_ok(y, n, what)
    if y2 is not None:
        _guards_ok(y2, n, what + " (y2)")
    sh = (c.cout, c.L * c.stride)
    return y[GUARD:GUARD + n].reshape(sh), None if y2 is None else y2[GUARD:GUARD + n].reshape(sh)


def _compare(c, y, y2, ref, refa, what, key):
    """the launch's outputs against (raw, activated): y2 set -> y raw, y2 activated; else y is the activated value when there is one"""
    if y2 is not None:
        e = max(rel_err(y, ref), rel_err(y2, refa))
    else:
        # the fused unit without an activated copy leaves the raw tensor; a conv with a consumer's snake and no y2 writes the activated value
        e = rel_err(y, refa if (refa is not None and c.kind != UNIT) else ref)
    _record(c, **{key: e})
    assert e < TOL, f"{what}: rel_err {e:.3e}"
    return e


# ---------------------------------------------------------------- dense, against float64
@gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.planes == 3], ids=[i for i, c in zip(IDS, CASES) if c.planes == 3])
def test_dense(c):
    what = _id(c)
    d = _inputs(c)
    # half of the snake cases hand over (alpha, beta) and let launch_snake_tables build the tables; the others pass tables
    raw = (c.L + c.cin) % 2 == 0
    y, y2 = _run(c, d, what, raw_tables=raw)
    ref, refa = _reference(c, d)
    _compare(c, y, y2, ref, refa, what, "rel_err")
    if c.opts.get("oracle"):
        _oracle_check(c, d, ref, what)


def _oracle_check(c, d, ref, what):
    """the CPU oracle on the same inputs, inside the same bound: the bound is f32 arithmetic's"""
    import oracle as O
    assert c.opts.get("act", 0) == 0 and d["scale"] is None and d["resid"] is None and d["post"] is None
    x = d["x"]
    if d["snake"] is not None:
        xs = np.zeros_like(x)
        O.olib.q3o_snake_beta(O.ptr(x), O.ptr(d["snake"][0]), O.ptr(d["snake"][1]), O.ptr(xs), c.cin, c.L)
        x = xs
    yo = np.zeros((c.cout, c.L * c.stride), dtype=np.float32)
    b = d["b"] if d["b"] is not None else np.zeros(c.cout, dtype=np.float32)
    if c.kind == TCONV:
        O.olib.q3o_causal_trans_conv1d(O.ptr(x), O.ptr(d["w"]), O.ptr(b), O.ptr(yo), c.cin, c.cout, c.L, c.k, c.stride)
    else:
        O.olib.q3o_causal_conv1d(O.ptr(x), O.ptr(d["w"]), O.ptr(b), O.ptr(yo), c.cin, c.cout, c.L, c.k, c.dil, 1)
    e = rel_err(yo, ref)
    _record(c, oracle_rel_err=e)
    assert e < TOL, f"{what}: the CPU oracle is {e:.3e} from float64"


ORACLE_CASES = [c for c in CASES if c.opts.get("oracle")]


def test_oracle_meets_the_same_bound():
    """no GPU: the oracle cases of the table, CPU oracle against the float64 definition"""
    assert len(ORACLE_CASES) >= 6 and {c.kind for c in ORACLE_CASES} == {CONV, TCONV} and any(c.opts.get("snake") for c in ORACLE_CASES)
    for c in ORACLE_CASES:
        d = _inputs(c)
        _oracle_check(c, d, _reference(c, d)[0], _id(c))


# ---------------------------------------------------------------- two-plane mode
@gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.planes == 2 and c.kind != UNIT], ids=[i for i, c in zip(IDS, CASES) if c.planes == 2 and c.kind != UNIT])
def test_two_plane_mode(c):
    what = _id(c)
    d = _inputs(c)
    y, y2 = _run(c, d, what)
    ref, refa = _reference(c, d, two_plane=True)
    _compare(c, y, y2, ref, refa, what, "rel_err_vs_mode")
    true, truea = _reference(c, d)
    _record(c, two_plane_distance_to_f64=rel_err(y, truea if (truea is not None and y2 is None) else true))      # recorded, not asserted


@gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.planes == 2 and c.kind == UNIT], ids=[i for i, c in zip(IDS, CASES) if c.planes == 2 and c.kind == UNIT])
def test_two_plane_unit_equals_its_two_launches(c):
    """The unit's two-plane form parks a re-split middle tensor, which float64 of "the mode" does not define on its own; its promise is the
    two-launch sequence's bits in the same mode. The distance to the true result is recorded."""
    what = _id(c)
    d = _inputs(c)
    y, y2 = _run(c, d, what, raw_tables=False)          # the same host-built tables as the two launches
    ty, ty2 = _two_launches(c, d, planes=2)
    assert (y.view(np.uint32) == ty.view(np.uint32)).all(), what
    if y2 is not None:
        assert (y2.view(np.uint32) == ty2.view(np.uint32)).all(), what
    c3 = c._replace(planes=3)
    ref, _ = _reference(c3, d)
    _record(c, two_plane_distance_to_f64=rel_err(y, ref))


@gpu
@pytest.mark.parametrize("k,cout,L", [(3, 64, 100), (5, 96, 300), (3, 256, 4000)])
def test_two_planes_asked_of_three_plane_taps(k, cout, L):
    """k in {3, 5} has no two-plane instance: planes = 2 must give the three-plane bits"""
    c = C(q.conv_path(cout, 48, L, k), cout, 48, L, k)
    d = _inputs(c)
    y3, _ = _run(c, d, _id(c))
    y2p, _ = _run(c, d, _id(c), planes=2)
    assert not (c.path & NP2) and (y3.view(np.uint32) == y2p.view(np.uint32)).all()


# ---------------------------------------------------------------- exact integers
def _sparse_rows(rng, rows, cols, nnz):
    """[rows][cols] bool, min(nnz, cols) per row: half of them walk over the columns row after row (every column is hit once rows * nnz / 2 >= cols),
    the others sit at seeded positions"""
    m = np.zeros((rows, cols), dtype=bool)
    n = min(nnz, cols)
    for r in range(rows):
        walk = (r * (n // 2) + np.arange(n // 2)) % cols
        m[r, walk] = True
        m[r, rng.choice(np.setdiff1d(np.arange(cols), walk), size=n - len(walk), replace=False)] = True
    return m


def _exact_inputs(c, variant, planes):
    """Integer inputs: every product and every partial sum, in any order, bias and residual included, is an integer (scaled by a power of two)
    below 2^24.  A: wide w, x in {0, +-1, +-2} (all weight planes); B: wide x, w = +-1 (all x planes); C: mid x mid"""
    rng = np.random.default_rng([c.cout, c.cin, c.L, c.k, c.stride, ord(variant), planes])
    taps = c.k // c.stride
    nnz = 8 if variant == "C" else 16
    wide = (1 << 14, 1 << 16) if planes == 2 else (1 << 17, 1 << 19)
    sign = lambda shape: rng.choice(np.array([-1, 1]), size=shape)
    if variant == "A":
        wv = (rng.integers(wide[0] // 2, wide[1] // 2, size=(c.cout, c.cin * taps)) * 2 + 1) * sign((c.cout, c.cin * taps))
        x = rng.integers(-2, 3, size=(c.cin, c.L))
    elif variant == "B":
        wv = sign((c.cout, c.cin * taps))
        x = rng.integers(-wide[1] + 1, wide[1], size=(c.cin, c.L))
    else:
        wv = rng.integers(1 << 8, 1 << 11, size=(c.cout, c.cin * taps)) * sign((c.cout, c.cin * taps))
        x = rng.integers(1 << 8, 1 << 10, size=(c.cin, c.L)) * sign((c.cin, c.L))
    mask = _sparse_rows(rng, c.cout, c.cin * taps, nnz)
    wr = np.where(mask, wv, 0).reshape(c.cout, c.cin, taps)          # per output row and phase: [cout][cin][taps]
    if c.kind == TCONV:
        # the same sparse rows for every phase, scattered into the checkpoint layout [cin][cout][k]: kernel index ph + (taps - 1 - tp) stride
        w = np.zeros((c.cin, c.cout, c.k), dtype=np.int64)
        for ph in range(c.stride):
            for tp in range(taps):
                w[:, :, ph + (taps - 1 - tp) * c.stride] = np.roll(wr[:, :, tp], ph, axis=0).T
    else:
        w = wr
    d = dict(x=x.astype(np.float32), w=w.astype(np.float32), snake=None, post=None)
    lim = 1 << 16
    d["b"] = rng.integers(-lim + 1, lim, size=c.cout).astype(np.float32) if c.opts.get("bias", True) else None
    d["scale"] = rng.choice(np.array([1.0, 0.5, 0.25], dtype=np.float32), size=c.cout) if c.opts.get("scale") else None
    d["resid"] = rng.integers(-lim + 1, lim, size=(c.cout, c.L * c.stride)).astype(np.float32) if c.resid else None
    # the test's own inputs: the magnitude bound that makes any summation order exact
    worst = np.abs(wr).reshape(c.cout, -1).sum(axis=1).max() * np.abs(x).max() + 2 * lim
    assert worst < (1 << 24), worst
    assert (mask.sum(axis=1) == min(nnz, c.cin * taps)).all()
    return d


EXACT_CASES = [c for c in CASES if c.kind != UNIT and not c.opts.get("act") and c.path & 31 not in (OUT1, OUT1_V4)]


@gpu
@pytest.mark.parametrize("c", EXACT_CASES, ids=[_id(c) for c in EXACT_CASES])
def test_exact(c):
    what = _id(c)
    ce = c._replace(opts={k: v for k, v in c.opts.items() if k in ("bias", "scale", "inplace", "y2")})
    for variant in (("A", "B") if c.planes == 2 else ("A", "B", "C")):
        d = _exact_inputs(ce, variant, c.planes)
        y, _ = _run(ce, d, f"{what} exact {variant}")
        ref, _ = _reference(ce, d)
        ref32 = ref.astype(np.float32)
        assert (ref32.astype(np.float64) == ref).all()
        bad = np.argwhere(y.view(np.uint32) != ref32.view(np.uint32))
        assert len(bad) == 0, f"{what} exact {variant}: {len(bad)} of {y.size} outputs differ from the integer result, first at {bad[0]}: " \
                              f"{y[tuple(bad[0])]!r} != {ref32[tuple(bad[0])]!r}"


# ---------------------------------------------------------------- same bits across kernels that promise it
def _two_launches(c, d, planes=3):
    """the residual unit as conv7 (+ middle snake) followed by the 1x1 with the in-place residual, both through q3_conv_ex"""
    n = c.cout * c.L
    mid, _, p1 = q.conv_ex(CONV, d["x"], d["w"], dil=c.dil, b=d["b"], post=_tables(d["mid"]), planes=planes)
    y = _buf(n, d["resid"]); y2 = _buf(n) if c.opts.get("y2") else None
    _, _, p2 = q.conv_ex(CONV, mid.reshape(c.cout, c.L), d["w2"], b=d["b2"], post=_tables(d["post"]), resid_in_place=True, planes=planes, y=y, y2=y2, y_front=GUARD)
    np_flag = NP2 if planes == 2 else 0
    assert p1 == G96_TM4 | np_flag and p2 == G96_6W | PRE | np_flag, (p1, p2)
    return y[GUARD:GUARD + n].reshape(c.cout, c.L), None if y2 is None else y2[GUARD:GUARD + n].reshape(c.cout, c.L)


@gpu
@pytest.mark.parametrize("c", [c for c in CASES if c.kind == UNIT and c.planes == 3], ids=[i for i, c in zip(IDS, CASES) if c.kind == UNIT and c.planes == 3])
def test_unit_equals_its_two_launches(c):
    d = _inputs(c)
    y, y2 = _run(c, d, _id(c), raw_tables=False)
    ty, ty2 = _two_launches(c, d)
    assert (y.view(np.uint32) == ty.view(np.uint32)).all(), _id(c)
    if y2 is not None:
        assert (y2.view(np.uint32) == ty2.view(np.uint32)).all(), _id(c)


@gpu
def test_lin_small_equals_the_tiled_kernel():
    """k_lin_small at L = 32 against the tiled kernel at L = 33 (one more column, the same first 32), column for column"""
    for planes in (3, 2):
        c32 = C((SMALL4 | SEG) | (NP2 if planes == 2 else 0), 64, 512, 32, 1, planes=planes, post=True, y2=True)
        d = _inputs(c32)
        c33 = C((G64x64 | CIS128 | SEG) | (NP2 if planes == 2 else 0), 64, 512, 33, 1, planes=planes, post=True, y2=True)
        d33 = dict(d, x=np.concatenate([d["x"], np.ones((512, 1), np.float32)], axis=1))
        a, a2 = _run(c32, d, _id(c32))
        b, b2 = _run(c33, d33, _id(c33))
        assert (a.view(np.uint32) == b[:, :32].view(np.uint32)).all() and (a2.view(np.uint32) == b2[:, :32].view(np.uint32)).all(), planes


@gpu
@pytest.mark.parametrize("c", [C(G96_6W, 96, 48, 1100, 7, 9, snake=True), C(G64x64 | CIS128, 64, 320, 65, 1), C(G96_TM4, 192, 32, 4097, 7, 3),
                               C(G64x64 | CIS128 | SEG, 128, 512, 33, 2, kind=TCONV, stride=2), C(MFMA32, 40, 80, 300, 3, 9, packed=False),
                               C(VALU, 8, 80, 129, 7, 9, packed=False), C(SMALL8 | SEG, 64, 1024, 31, 1)], ids=_id)
def test_arithmetic_does_not_depend_on_position(c):
    """a conv at length L against the same conv at L + 128 on the common prefix: other tiles, other tile counts, the same bits"""
    d = _inputs(c)
    c2 = c._replace(L=c.L + 128, path=_table_path(c._replace(L=c.L + 128)))
    ext = np.random.default_rng(5).standard_normal((c.cin, 128)).astype(np.float32)
    d2 = dict(d, x=np.concatenate([d["x"], ext], axis=1))
    a, _ = _run(c, d, _id(c))
    b, _ = _run(c2, d2, _id(c2))
    n = c.L * c.stride
    assert (a.view(np.uint32) == b[:, :n].view(np.uint32)).all()


# ---------------------------------------------------------------- refusals
@gpu
@pytest.mark.parametrize("why", REFUSALS, ids=lambda w: "-".join(f"{k}{v}" for k, v in w.items()))
def test_unit_refusals(why):
    Cc, L, dil = why.get("C", 96), why.get("L", 4096), why.get("dil", 1)
    c = C(0, Cc, Cc, L, 7, dil, kind=UNIT, packed=why.get("packed", True), y2=not why.get("y2_is_x"), post=True)
    d = _inputs(c)
    n = Cc * L
    y = _buf(n, d["resid"]); y2 = None if why.get("y2_is_x") else _buf(n)
    before = y.copy()
    with pytest.raises(_lib.Q3Error) as e:
        q.conv_ex(UNIT, d["x"], d["w"], dil=dil, b=d["b"], w2=d["w2"], b2=d["b2"], mid=_tables(d["mid"]), post=_tables(d["post"]), packed=c.packed,
                  y=y, y2=y2, y_front=GUARD, y2_is_x=bool(why.get("y2_is_x")))
    assert e.value.status == 7 and e.value.path == 0 and "refused" in str(e.value)
    assert (y.view(np.uint32) == before.view(np.uint32)).all()
    assert y2 is None or (y2.view(np.uint32) == SENT.view(np.uint32)).all()


@gpu
def test_conv_refusals():
    x = np.ones((16, 100), np.float32)
    for (k, dil) in ((8, 1), (7, 10)):
        y = _buf(64 * 100)
        with pytest.raises(_lib.Q3Error) as e:
            q.conv_ex(CONV, x, np.ones((64, 16, k), np.float32), dil=dil, y=y, y_front=GUARD)
        assert e.value.status == 7 and e.value.path == 0 and (y.view(np.uint32) == SENT.view(np.uint32)).all()
    with pytest.raises(_lib.Q3Error) as e:          # packed weights need cout % 32 == 0 and cin % 16 == 0
        q.conv_ex(CONV, np.ones((24, 100), np.float32), np.ones((40, 24, 3), np.float32))
    assert e.value.status == 7


# ---------------------------------------------------------------- snake tables
@gpu
def test_snake_tables_from_alpha_beta():
    """launch_snake_tables: a = exp(alpha), 1 / b = 1 / (exp(beta) + 1e-9), seen through a 1 x 1 identity conv with snake on load"""
    cin = 64
    rng = np.random.default_rng(3)
    x = rng.standard_normal((cin, 50)).astype(np.float32) * 3
    al = rng.uniform(-0.5, 0.5, cin).astype(np.float32); be = rng.uniform(-0.5, 0.5, cin).astype(np.float32)
    w = np.eye(cin, dtype=np.float32).reshape(cin, cin, 1)
    a, _, _ = q.conv_ex(CONV, x, w, snake=(al, be), snake_raw=True)
    b, _, _ = q.conv_ex(CONV, x, w, snake=_tables((al, be)))
    ref = snake_ref(x.astype(np.float64), al.astype(np.float64), be.astype(np.float64))
    ea, eb = rel_err(a.reshape(cin, 50), ref), rel_err(b.reshape(cin, 50), ref)
    print(f"snake tables: device tables {ea:.3e}, host tables {eb:.3e}")
    assert ea < 1e-6 and eb < 1e-6          # one rounding of exp and of the quotient (2^-24 each) through a slope <= 2 |x| a / b


# ---------------------------------------------------------------- norm_c / dwconv7
NORM_TOL = 4e-6          # test_fused_residual_rmsnorm_f32's absolute figure, at unit scale


@gpu
@pytest.mark.parametrize("layernorm", [False, True], ids=["rms", "ln"])
@pytest.mark.parametrize("Cn", [512, 1024, 96, 100])
def test_norm_c(Cn, layernorm):
    """C = 1024 / 512: k_norm_c2<.., 64 | 32>; else k_norm_c. float64 of E[x^2] - mean^2 (candle's formula and the oracle's)"""
    for L in (1, 15, 16, 17, 33):
        rng = np.random.default_rng([Cn, L, int(layernorm)])
        x = (rng.standard_normal((Cn, L)) + rng.uniform(-1, 1, (1, L))).astype(np.float32)          # |mean| <= std: the formula is well conditioned
        w = (1.0 + 0.1 * rng.standard_normal(Cn)).astype(np.float32)
        b = (0.1 * rng.standard_normal(Cn)).astype(np.float32) if layernorm else None
        eps = 1e-6 if layernorm else 1e-5
        y = _buf(Cn * L)
        q.norm_c(x, w, b, eps, y=y, y_front=GUARD)
        _guards_ok(y, Cn * L, f"norm_c C={Cn} L={L}")
        x8 = x.astype(np.float64)
        if layernorm:
            mean = x8.mean(axis=0); var = (x8 * x8).mean(axis=0) - mean * mean
            ref = (x8 - mean) / np.sqrt(var + eps) * w[:, None] + b[:, None]
        else:
            ref = x8 / np.sqrt((x8 * x8).mean(axis=0) + eps) * w[:, None]
        err = float(np.abs(y[GUARD:GUARD + Cn * L].reshape(Cn, L) - ref).max())
        RESULTS.setdefault(f"norm_c-{'ln' if layernorm else 'rms'}-C{Cn}", {"path": f"k_norm_c{'2' if Cn in (512, 1024) else ''} {'LayerNorm' if layernorm else 'RMSNorm'}"})[f"abs_err_L{L}"] = err
        print(f"norm_c C={Cn} L={L} layernorm={layernorm}: abs err {err:.3e}")
        assert err < NORM_TOL, (Cn, L, err)


def _fma32(a, b, c):
    """float32 fma(a, b, c) of float32 arrays, exactly: a * b is exact in float64 (24 + 24 bits); the sum with c is taken with its rounding error
    (TwoSum), and where the float64 sum sits exactly on a float32 tie the error term decides the direction instead of round-to-even"""
    p = a.astype(np.float64) * b.astype(np.float64); c = c.astype(np.float64)
    s = p + c
    t = s - p
    e = (p - (s - t)) + (c - t)                       # exact: s + e == p + c
    r = s.astype(np.float32)
    r8 = r.astype(np.float64)
    n = np.where(s > r8, np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf)))
    tie = (s == (r8 + n.astype(np.float64)) * 0.5) & (e != 0) & (s != r8)
    return np.where(tie, np.where(e > 0, np.maximum(r, n), np.minimum(r, n)), r).astype(np.float32)


@gpu
@pytest.mark.parametrize("Cn", [512, 96, 100])
def test_dwconv7(Cn):
    """an fmaf chain over the 7 taps, ascending, then + bias: bit-equal to the float32 fma emulation"""
    for L in (1, 5, 15, 16, 17, 33, 300):
        rng = np.random.default_rng([Cn, L])
        x = rng.standard_normal((Cn, L)).astype(np.float32); w = (rng.standard_normal((Cn, 7)) / math.sqrt(7)).astype(np.float32)
        b = rng.standard_normal(Cn).astype(np.float32)
        y = _buf(Cn * L)
        q.dwconv7(x, w, b, y=y, y_front=GUARD)
        _guards_ok(y, Cn * L, f"dwconv7 C={Cn} L={L}")
        acc = np.zeros((Cn, L), dtype=np.float32)
        for kk in range(7):
            sh = 6 - kk
            if sh < L:
                acc[:, sh:] = _fma32(np.broadcast_to(w[:, kk:kk + 1], (Cn, L - sh)), x[:, :L - sh], acc[:, sh:])
        ref = acc + b[:, None]
        got = y[GUARD:GUARD + Cn * L].reshape(Cn, L)
        bad = int((got.view(np.uint32) != ref.view(np.uint32)).sum())
        assert bad == 0, (Cn, L, bad)
