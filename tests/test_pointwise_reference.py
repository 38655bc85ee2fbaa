"""What tests/test_gpu_pointwise_ops.py rests on and a CPU can check (tables and references: tests/pointwise_cases.py): the exact float32
fma of the restatement against rational arithmetic; the restatement of sin_sq against float64 (B_SIN) and its evenness; the exactness the
routine's comment claims for k PI_A / k PI_B; that the table bites (mutations of the restatement); that a contracted snake_f shows on
the generic rows; the CPU oracle's q3o_snake_beta on the same table; the shapes against the dispatcher and the call-site table; every
frozen figure against its re-measurement.

Two of the mutations cannot do what was expected of them, for reasons of arithmetic and not of the table (figures in
test_the_table_bites): the r^11 coefficient changed in its last place changes NO float32 result at all (its term is at most 3.6e-6, one
ulp of the coefficient moves it by 2e-13), and rint replaced by truncation leaves k unchanged wherever frac(|t| / pi) < 1/2 — half of
all arguments — and is invisible on the rows next to (k + 1/2) pi, where sin^2 is flat: it moves 36 % of the rows, every one it can."""
import ctypes
import ctypes.util
import fractions
import math

import numpy as np

import qwen3_tts_rs_amd as q
import pointwise_cases as P
from pointwise_cases import f32, f64

F = fractions.Fraction


# ---------------------------------------------------------------- the exact fma
def _round_f32(v):
    """a rational rounded to the nearest float32, ties to even (normal range)"""
    if v == 0:
        return f32(0)
    sign = -1 if v < 0 else 1
    v = abs(v)
    e = v.numerator.bit_length() - v.denominator.bit_length()          # 2^(e - 1) < v < 2^(e + 1)
    if v < F(2) ** e:
        e -= 1
    assert F(2) ** e <= v < F(2) ** (e + 1) and -126 <= e <= 126
    scaled = v / F(2) ** (e - 23)                                        # in [2^23, 2^24)
    n = scaled.numerator // scaled.denominator
    rem = scaled - n
    if rem > F(1, 2) or (rem == F(1, 2) and n & 1):
        n += 1
    return f32(sign * math.ldexp(n, e - 23))


def _double_rounding_cases():
    """a b lies exactly on a float32 tie and c, far below an ulp of float64's sum, decides the direction: float64 a b + c rounds onto the
    tie, the cast then rounds to even — wrong for half of the signs"""
    a, b, c = [], [], []
    for i in (-20, -3, 0, 5, 30):
        for j in (-7, 0, 11):
            for m in (1, 3, 1001, 4095):
                for sc in (-60, -45, -35):
                    for sg in (1.0, -1.0):
                        # (1 + m 2^-12)(1 + 2^-12) = 1 + (m + 1) 2^-12 + m 2^-24: bit 2^-24 is set for odd m: a tie of the 2^-23 grid
                        a.append(math.ldexp(1.0 + m * 2.0 ** -12, i)); b.append(math.ldexp(1.0 + 2.0 ** -12, j)); c.append(sg * math.ldexp(1.0, i + j + sc))
    return np.array(a, dtype=f32), np.array(b, dtype=f32), np.array(c, dtype=f32)


def test_fma32_against_rational_arithmetic():
    rng = np.random.default_rng(1)
    n = 3000
    a = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(f32)
    b = (rng.standard_normal(n) * np.exp2(rng.integers(-20, 20, n))).astype(f32)
    c = np.where(rng.integers(0, 2, n) == 1, -(a.astype(f64) * b.astype(f64)) * (1 + rng.standard_normal(n) * 1e-6), rng.standard_normal(n)).astype(f32)   # cancellation too
    da, db, dc = _double_rounding_cases()
    a = np.concatenate([a, da]); b = np.concatenate([b, db]); c = np.concatenate([c, dc])
    got = P.fma32(a, b, c)
    want = np.array([_round_f32(F(float(x)) * F(float(y)) + F(float(z))) for x, y, z in zip(a, b, c)], dtype=f32)
    assert (got.view(np.uint32) == want.view(np.uint32)).all()
    # the constructed cases are what they claim: the plain float64 product-sum, cast, gets some of them wrong
    naive = (da.astype(f64) * db.astype(f64) + dc.astype(f64)).astype(f32)
    wrong = int((naive.view(np.uint32) != want[n:].view(np.uint32)).sum())
    assert wrong >= len(da) // 8, wrong


# ---------------------------------------------------------------- the table
def test_table_contents():
    tab = P.snake_table()
    at = np.abs(tab.t); pos = tab.t[:tab.half]
    b = P.bucket_of(tab.t)
    rnd = tab.kind == P.KINDS.index("random")
    for i in range(5):
        assert (rnd & (b == i) & (tab.t > 0)).sum() >= 1000 and (rnd & (b == i) & (tab.t < 0)).sum() >= 1000, P.BUCKET_NAMES[i]
    assert (b == 5).sum() >= 6000 and at.max() < 2.0 ** 17 and at[at > 0].min() >= 2.0 ** -20
    have = set(np.abs(pos).tolist())
    for k in (1, 2, 3, 100, 1303, 2606, P.K_MAX):
        for c in (f32(k * math.pi), f32((k + 0.5) * math.pi)):
            assert {float(np.nextafter(c, f32(0))), float(c), float(np.nextafter(c, f32(np.inf)))} <= have, k
    assert {float(np.nextafter(P.SWITCH, f32(0))), 8192.0, float(np.nextafter(P.SWITCH, f32(np.inf))), 0.0} <= have
    # rint's ties: fl32(t / pi) exactly k + 1/2, for even and odd k, spread over the range
    prod = np.abs(tab.t * P.INV_PI)[at < P.SWITCH]
    tie = prod[(prod % 1) == 0.5]
    kk = np.floor(tie)
    assert len(tie) >= 1000 and (kk % 2 == 0).sum() >= 300 and (kk % 2 == 1).sum() >= 300 and kk.min() < 50 and kk.max() > 2500
    # the mirrored half: the same x, -a, exactly -t
    assert (tab.x[:tab.half].view(np.uint32) == tab.x[tab.half:].view(np.uint32)).all() and (tab.t[tab.half:] == -tab.t[:tab.half]).all()
    assert (tab.a[tab.grp[tab.half:]] == -tab.a[tab.grp[:tab.half]]).all()
    # one ulp of sin^2 moves y on the power-of-two rows: |x| <= 2^-12, ib = 1
    pw = tab.kind != P.KINDS.index("generic")
    assert (np.abs(tab.x[pw]) <= 2.0 ** -12).all() and (tab.ib[tab.grp[pw]] == 1).all()
    assert np.rint(at[at < P.SWITCH] * P.INV_PI).max() == P.K_MAX + 1          # 8192 / pi = 2607.6


def test_pack_places_every_row_once():
    tab = P.snake_table()
    for C, L in ((16, 2048), (512, 32), (1, 8192), (96, 4096)):
        seen = np.zeros(len(tab.x), dtype=np.int64)
        for X, A, IB, I in P.pack(tab.x, tab.grp, tab.a, tab.ib, C, L):
            m = I >= 0
            seen[I[m]] += 1
            assert (X[m] == tab.x[I[m]]).all() and (X[~m] == 0).all()
            ch = np.nonzero(m.any(axis=1))[0]
            assert all((tab.grp[I[c][m[c]]] == tab.grp[I[c][0]]).all() and A[c] == tab.a[tab.grp[I[c][0]]] and IB[c] == tab.ib[tab.grp[I[c][0]]] for c in ch)
        assert (seen == 1).all()


# ---------------------------------------------------------------- the restatement
def test_restatement_against_float64_and_frozen_figures():
    b = P.measure_b_sin()
    d = P.measure_d_ref_sin2()
    da, dib = P.measure_d_ref_tables()
    print(f"B_SIN {b:.4e} (frozen {P.B_SIN:.3e}); D_REF_SIN2 {d:.4e} (frozen {P.D_REF_SIN2:.3e}); tables {da:.4e} / {dib:.4e}")
    for got, const in ((b, P.B_SIN), (d, P.D_REF_SIN2), (da, P.D_REF_TAB_A), (dib, P.D_REF_TAB_IB)):
        assert 0.5 * const <= got <= const <= 1.2 * got, (got, const)
    tab = P.snake_table()
    m = np.abs(tab.t) < P.SWITCH
    e = np.abs(P.sin_sq32(tab.t[m]).astype(f64) - P.sin2_64(tab.t[m]))
    bk = P.bucket_of(tab.t[m])
    print("restatement, worst |sin^2 error| per bucket: " + ", ".join(f"{P.BUCKET_NAMES[i]} {e[bk == i].max():.3e}" for i in range(5)))
    assert e.max() <= P.B_SIN


def test_restatement_is_even():
    tab = P.snake_table()
    m = np.abs(tab.t) < P.SWITCH
    assert (P.sin_sq32(tab.t[m]).view(np.uint32) == P.sin_sq32(-tab.t[m]).view(np.uint32)).all()
    a, ib = tab.a[tab.grp], tab.ib[tab.grp]
    y = P.snake32(tab.x, a, ib)
    mm = m[:tab.half]
    assert (P.canon_bits(y[:tab.half][mm]) == P.canon_bits(y[tab.half:][mm])).all()


def test_reduction_products_are_exact():
    """the routine's comment: k PI_A (and k PI_B) exact for |k| < 2^13 — checked for every k the table reaches below 8192"""
    tab = P.snake_table()
    k = np.unique(np.abs(np.rint(tab.t[np.abs(tab.t) < P.SWITCH] * P.INV_PI))).astype(f64)
    assert k.max() == P.K_MAX + 1 and len(k) == P.K_MAX + 2 and k.max() < 2 ** 13
    for c in (P.PI_A, P.PI_B):
        p = k * f64(c)                                        # exact in float64: 12 + 24 bits
        assert (p.astype(f32).astype(f64) == p).all()
    assert all(F(int(kk)) * F(float(P.PI_A)) == F(float(f32(kk * f64(P.PI_A)))) for kk in (1.0, 1303.0, 2608.0))
    # and the three constants are pi to well below what k = 2607 can show in float32 (2608 x 4e-15 = 1e-11 against the 3e-8 of r's own rounding)
    assert abs(F(float(P.PI_A)) + F(float(P.PI_B)) + F(float(P.PI_C)) - F(math.pi)) < F(4, 10 ** 15)


def _pi_b_low_bit_cleared():
    u = int(P.PI_B.view(np.uint32))
    return np.uint32(u & (u - 1)).view(f32)


def test_the_table_bites():
    """mutations of the restatement over the rows of [64, 8192): the fraction whose bits move and the worst sin^2 error"""
    tab = P.snake_table()
    at = np.abs(tab.t)
    t = tab.t[(at >= 64) & (at < P.SWITCH)]
    base = P.sin_sq32(t)
    ref = P.sin2_64(t)

    def run(**kw):
        mu = P.sin_sq32(t, **kw)
        moved = mu.view(np.uint32) != base.view(np.uint32)
        return moved, float(np.abs(mu.astype(f64) - ref).max())
    for name, kw in (("third reduction term dropped", dict(terms=2)), ("PI_B's lowest set bit cleared", dict(pi_b=_pi_b_low_bit_cleared()))):
        moved, worst = run(**kw)
        print(f"{name}: {moved.mean():.3f} of the rows move, worst error {worst:.3e} = {worst / P.B_SIN:.0f} B_SIN")
        assert moved.mean() > 0.5 and worst > 4 * P.B_SIN, name
    # rint -> trunc: k is unchanged where frac(|t| / pi) < 1/2, and next to (k + 1/2) pi the polynomial's error at |r| just above pi / 2 is
    # below an ulp of sin^2 ~ 1. Every row that CAN move does: all with frac in [0.55, 0.95]; none with frac in (0.01, 0.49) (right above k pi
    # the float32 quotient can fall below k)
    moved, worst = run(rnd=np.trunc)
    fr = np.abs(t.astype(f64)) / math.pi % 1.0
    print(f"rint -> trunc: {moved.mean():.3f} of the rows move, worst error {worst:.3e} = {worst / P.B_SIN:.0f} B_SIN")
    assert moved[(fr >= 0.55) & (fr <= 0.95)].all() and not moved[(fr > 0.01) & (fr < 0.49)].any()
    assert moved.mean() > 1 / 3 and worst > 4 * P.B_SIN
    # the r^11 coefficient: its last place is invisible in float32 (no row moves: not a gap of the table, the results do not depend on it);
    # the coefficient as a whole is needed: without it every row with |r| > 1.2 moves and the worst error is 20 B_SIN
    moved, worst = run(c11=np.nextafter(P.POLY[0], f32(0)))
    assert not moved.any() and worst <= P.B_SIN
    moved, worst = run(c11=f32(0))
    r = np.abs((t.astype(f64) + math.pi / 2) % math.pi - math.pi / 2)
    print(f"r^11 term dropped: {moved.mean():.3f} of the rows move, worst error {worst:.3e} = {worst / P.B_SIN:.0f} B_SIN")
    assert moved[r > 1.2].all() and moved.mean() > 1 / 3 and worst > 4 * P.B_SIN


def test_a_contracted_snake_shows_on_the_generic_rows():
    tab = P.snake_table()
    a, ib = tab.a[tab.grp], tab.ib[tab.grp]
    y = P.snake32(tab.x, a, ib); yc = P.snake32(tab.x, a, ib, contracted=True)
    g = tab.kind == P.KINDS.index("generic")
    diff = P.canon_bits(y) != P.canon_bits(yc)
    print(f"x + s ib as one fma: {diff[g].mean():.3f} of the generic rows change, {int(diff[~g].sum())} of the others")
    assert diff[g].mean() > 0.02 and not diff[~g].any()
    # per generic group: each (a, ib) pair shows it
    assert all(diff[tab.grp == gg].any() for gg in np.unique(tab.grp[g]))


# ---------------------------------------------------------------- the oracle on the table
def test_oracle_snake_beta_on_the_table():
    """q3o_snake_beta takes (alpha, beta): the positive-a half of the table with alpha = log a, beta = -log ib; t is the float32 product
    with the a the oracle itself forms — libm's expf of the float32 alpha — so the special rows move by a few ulps of t, which a sinf-based
    routine does not care about. Bound: 4 D_REF_SIN2 |ib| + one rounding of y."""
    import oracle as O
    tab = P.snake_table()
    G = len(tab.a) // 2
    assert (tab.a[:G] > 0).all()
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype = ctypes.c_float; libm.expf.argtypes = [ctypes.c_float]
    expf = lambda v: f32(libm.expf(float(v)))
    alpha = np.log(tab.a[:G].astype(f64)).astype(f32)
    beta = np.where(tab.ib[:G] == 1, 0.0, -np.log(tab.ib[:G].astype(f64))).astype(f32)
    a_o = np.array([expf(v) for v in alpha], dtype=f32)
    ib_o = np.array([f32(1.0) / (expf(v) + f32(1e-9)) for v in beta], dtype=f32)
    assert (np.abs(a_o / tab.a[:G] - 1) < 1e-6).all() and (ib_o[:len(P.POW2_E)] == 1).all()
    packs = P.pack(tab.x, tab.grp, a_o, ib_o, 64, 4096)
    assert len(packs) == 1
    X, A, IB, I = packs[0]
    al = np.zeros(64, dtype=f32); be = np.full(64, 30.0, dtype=f32)          # spare channels: x = 0
    for c in range(64):
        if (I[c] >= 0).any():
            g = tab.grp[I[c][0]]; al[c] = alpha[g]; be[c] = beta[g]
    Y = np.zeros_like(X)
    O.olib.q3o_snake_beta(O.ptr(X), O.ptr(al), O.ptr(be), O.ptr(Y), 64, 4096)
    m = I >= 0
    Am = np.broadcast_to(A[:, None], X.shape)[m]; IBm = np.broadcast_to(IB[:, None], X.shape)[m]
    y64 = P.snake64(X[m], Am, IBm)
    ratio = np.abs(Y[m].astype(f64) - y64) / (4 * P.D_REF_SIN2 * np.abs(IBm.astype(f64)) + 2.0 ** -24 * np.abs(y64))
    print(f"oracle on {int(m.sum())} rows: worst deviation {ratio.max():.3f} of 4 D_REF_SIN2 |ib| + one rounding")
    assert int(m.sum()) == tab.half and ratio.max() <= 1.0


# ---------------------------------------------------------------- shapes, paths, sites
def test_shapes_reach_their_paths_and_cover_every_site():
    for s in P.SHAPES.values():
        if s.kind == P.UNIT:
            got = q.resunit_path(s.C, s.L, 1, True, False, 3)
        else:
            cout = 1 if s.name.startswith("out1") else s.C
            got = q.conv_path(cout, s.C, s.L, s.k, 1, 1, s.packed, False, 3, True)
        assert got == s.path, f"{s.name}: dispatches to {q.conv_path_name(got)} ({got}), the table names {q.conv_path_name(s.path)}"
        assert s.C * s.L >= 16384 or s.name.startswith("out1")
    assert q.conv_path_name(P.SHAPES["x3"].path) == "k_conv_bf16x3<64co x 64t>" and q.conv_path_name(P.SHAPES["x3_cis128"].path).endswith("CIS=128")
    assert q.conv_path_name(P.SHAPES["small"].path).startswith("k_lin_small_bf16x3<4>")
    # the call sites, by kernel template and role: twelve of snake_f, four of conv_act
    load = {"k_conv1d", "k_conv1d_mfma", "k_conv_bf16x3", "k_lin_small_bf16x3", "k_conv_out1", "k_conv_out1_v4"}
    post = {"k_conv1d", "k_conv1d_mfma", "k_conv_bf16x3", "k_lin_small_bf16x3", "k_resunit_bf16x3"}
    assert set(P.SNAKE_SITES) == {(k, "load") for k in load} | {(k, "post") for k in post} | {("k_resunit_bf16x3", "mid")} and len(P.SNAKE_SITES) == 12
    assert set(P.ACT_SITES) == {(k, "act") for k in ("k_conv1d", "k_conv1d_mfma", "k_conv_bf16x3", "k_lin_small_bf16x3")}
    for sites in (P.SNAKE_SITES, P.ACT_SITES):
        for (kernel, role), shapes in sites.items():
            assert shapes and all(P.KERNEL_OF[P.SHAPES[n].path & 31] == kernel for n in shapes), (kernel, role)
    # both stagings of k_conv_bf16x3 run: 32-channel stages and CIS = 128
    assert {P.SHAPES[n].path & P.CIS128 for n in P.SNAKE_SITES[("k_conv_bf16x3", "load")]} == {0, P.CIS128}
    assert set(P.SHAPES) == {n for shapes in list(P.SNAKE_SITES.values()) + list(P.ACT_SITES.values()) for n in shapes}


def test_channel_table_is_safe_for_the_planes():
    """no inf / NaN, |v| <= 2^100, and every bf16 plane of every value finite and normal (or zero)"""
    from test_gpu_conv_ops import bf16_rne
    for v in (P.channel_table(), P.snake_table().x, P.act_table().v):
        assert np.isfinite(v).all() and (np.abs(v) <= 2.0 ** 100).all()
        h = bf16_rne(v); m = bf16_rne(v - h); lo = (v - h) - m
        assert np.isfinite(h).all() and (h.astype(f64) + m.astype(f64) + lo.astype(f64) == v.astype(f64)).all()
        assert (bf16_rne(lo) == lo).all()
        tiny = np.finfo(f32).tiny
        for p in (h, m, lo):
            assert ((p == 0) | (np.abs(p) >= tiny)).all()
    assert len(set(P.channel_table().view(np.uint32).tolist())) > 16000


# ---------------------------------------------------------------- activations
def test_act_table_and_frozen_figures():
    tab = P.act_table()
    for b, name in enumerate(tab.names):
        v = np.abs(tab.v[tab.bucket == b])
        assert name == "zero" or (v.min() > 0 and v.max() <= 8 * v.min() * (1 + 1e-6)), name
        assert name == "zero" or len(set(np.sign(tab.v[tab.bucket == b]).tolist())) == 1, name
    assert {-100.0, 100.0, 0.0}.issubset(set(tab.v.tolist())) and tab.v.min() <= -108 and np.signbit(tab.v[tab.v == 0]).any()
    assert ((tab.v > -1.0001e-3) & (tab.v < -0.9999e-6)).sum() >= 1600
    got = P.measure_d_ref_act()
    assert set(got) == set(P.D_REF_ACT) == set(P.ACTS) - {3}
    for act, figs in got.items():
        assert len(figs) == len(P.D_REF_ACT[act]) == len(tab.names)
        for name, g, c in zip(tab.names, figs, P.D_REF_ACT[act]):
            assert (g == 0 and c == 0) or 0.5 * c <= g <= c <= 1.2 * g, (act, name, g, c)
    # float64 of sigmoid(-100) is 3.7e-44: below float32's normal range, and float32 arithmetic gives 0 (expf overflows to inf)
    assert P.act32(f32(-100.0), 5) == 0 and 0 < P.act64(f32(-100.0), 5) < 1e-43
