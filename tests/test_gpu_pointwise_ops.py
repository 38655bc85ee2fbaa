"""Op-level tests of the vocoder's pointwise nonlinearities over their whole argument range: SnakeBeta (snake_f / sin_sq) at each of the
twelve places q3_kernels_codec.hip inlines it, and conv_act's activations at its four. Tables, references and the call-site table:
tests/pointwise_cases.py; what a CPU can check of them: tests/test_pointwise_reference.py.

Each site is observed through an identity conv (q3_conv_ex, three planes): test_channel_is_exact asserts first, per kernel path, that the
same launch without a nonlinearity returns a table of full 24-bit mantissas bit for bit. Then, per site:
  * SnakeBeta, |t| < 8192: y equals the float32 restatement BIT FOR BIT; the mirrored row (-a) gives the same bits;
    |t| >= 8192 (sinf): |y - y64| <= 4 D_REF_SIN2 |ib| + one rounding of y;
  * every site gives every other site's bits on every row, the sinf rows included;
  * activations: per bucket max |y - y64| / max |y64| <= 4 D_REF_ACT[act][bucket]; ReLU bit-exact; the same bits from every site;
  * sentinels in front of and behind y and y2 survive (and no output is left unwritten: the results start out as sentinels);
  * launch_snake_tables over alpha, beta in [-6, 6] and beta = -25: the (a, 1 / b) pair the kernel built is IDENTIFIED — the one pair
    of float32 within 8 ulps of the float64 values whose restatement reproduces every observed y bit — and held to float64 within
    4 x what numpy float32 deviates.
The out1 kernels run with act = 0: their production clamp would cut y = x + sin^2 at 1. Two-plane mode is not exact through the channel
and not covered. Figures go to pointwise_ops.json in the report directory of the GPU tests.

Measured on the MI355X: all twelve sites (fourteen runs) give the restatement's bits on the 82 344 rows with |t| < 8192 and each other's on
all 93 412; worst |sin^2 error| in units of B_SIN per bucket of |t| (power-of-two rows, y's rounding included) 0.81, 0.83, 0.85, 1.03,
0.99, and 0.40 on the sinf rows, which lie at 0.25 of their bound; activations at most 1.25 D_REF_ACT (GELU, -[1/4, 2]; ELU 1.00, sigmoid
and tanh(ReLU) 0.91; bound 4); the snake tables 0.46 (a) and 0.86 (1 / b) of numpy float32's deviation (bound 4). With the third
reduction term dropped in a scratch build every site test fails (63 824 rows, 3.9e-4); with snake_f written as plain x + s * ib every
site test fails on the 1806 generic rows a single fma changes — and every test the suite had before passes with both."""
import collections

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import pointwise_cases as P
from pointwise_cases import f32, f64
from test_gpu_conv_ops import GUARD, SENT, _buf, _guards_ok
from test_gpu_parity import _dump          # the report directory of the GPU tests

gpu = pytest.mark.gpu
RESULTS = collections.OrderedDict()
GPU_RAN = []


@pytest.fixture(scope="module", autouse=True)
def _dump_results():
    yield
    if GPU_RAN:
        _dump("pointwise_ops.json", RESULTS)


def _launch(s, x, what, *, role=None, pair=None, act=0):
    """One q3_conv_ex launch of shape s's identity conv over x [C][L]. role: None (the bare channel), "act", or where the SnakeBeta
    `pair` (a [C], ib [C]) goes: "load", "post", "mid". -> the observed values [cout][L]; path and guards asserted."""
    w = P.identity_w(s)
    cout = w.shape[0]
    n = cout * s.L
    kw = dict(packed=s.packed, planes=3, act=act, y_front=GUARD)
    unit = s.kind == P.UNIT
    if unit:
        zero = np.zeros(s.C, dtype=f32)
        kw.update(w2=np.eye(s.C, dtype=f32).reshape(s.C, s.C, 1), mid=pair if role == "mid" else (zero, zero))       # a = 0, ib = 0: x + sin_sq(0) 0
    elif role == "mid":
        raise AssertionError("mid is the unit's")
    if role == "load":
        assert not unit          # the unit takes an activated operand: its producer's epilogue is the site
        kw["snake"] = pair
    y = _buf(n, np.zeros(n, dtype=f32) if unit else None)          # the unit adds onto a zero residual in place; elsewhere: sentinels
    y2 = None
    if role == "post":
        kw["post"] = pair
        y2 = _buf(n)
    _, _, path = q.conv_ex(s.kind, x, w, y=y, y2=y2, **kw)
    GPU_RAN.append(1)
    assert path == s.path, f"{what}: ran {q.conv_path_name(path)} ({path}), the table names {q.conv_path_name(s.path)}"
    _guards_ok(y, n, what)
    out = y[GUARD:GUARD + n].reshape(cout, s.L)
    if y2 is not None:
        _guards_ok(y2, n, what + " (y2)")
        # the raw tensor beside the activated one is the channel itself
        assert (P.canon_bits(out) == P.canon_bits(x[:cout])).all(), f"{what}: the raw output beside the activated one is not x"
        out = y2[GUARD:GUARD + n].reshape(cout, s.L)
    assert not (out.view(np.uint32) == SENT.view(np.uint32)).any(), f"{what}: outputs left unwritten"
    return out


def _is_out1(s):
    return s.name.startswith("out1")


def _run_flat(s, v, what, **kw):
    """a flat table through shape s (the out1 kernels observe channel 0 only) -> the results in table order"""
    res = np.full(len(v), np.nan, dtype=f32)
    for X, I in P.pack_flat(v, 1 if _is_out1(s) else s.C, s.L):
        if _is_out1(s):
            X = np.concatenate([X, np.zeros((s.C - 1, s.L), dtype=f32)]); I = np.concatenate([I, np.full((s.C - 1, s.L), -1)])
        out = _launch(s, X, what, **kw)
        m = I[:out.shape[0]] >= 0
        res[I[:out.shape[0]][m]] = out[m]
    assert not np.isnan(res).any()
    return res


# ---------------------------------------------------------------- the channel
@gpu
@pytest.mark.parametrize("name", list(P.SHAPES))
def test_channel_is_exact(name):
    s = P.SHAPES[name]
    v = P.channel_table()
    got = _run_flat(s, v, f"channel {name}")
    bad = np.nonzero(P.canon_bits(got) != P.canon_bits(v))[0]
    assert len(bad) == 0, f"{name}: {len(bad)} of {len(v)} values do not pass the identity conv unchanged, first {v[bad[0]]!r} -> {got[bad[0]]!r}"


# ---------------------------------------------------------------- SnakeBeta
_SNAKE = {}


def _snake_result(site, name):
    """the whole table through one site (memoised: the cross-site test shares the launches)"""
    key = (site, name)
    if key in _SNAKE:
        return _SNAKE[key]
    s = P.SHAPES[name]
    tab = P.snake_table()
    assert P.KERNEL_OF[s.path & 31] == site[0]
    what = f"{site[0]} {site[1]} ({name})"
    res = np.full(len(tab.x), np.nan, dtype=f32)
    for X, A, IB, I in P.pack(tab.x, tab.grp, tab.a, tab.ib, 1 if _is_out1(s) else s.C, s.L):
        if _is_out1(s):
            pad = s.C - 1
            X = np.concatenate([X, np.zeros((pad, s.L), dtype=f32)]); I = np.concatenate([I, np.full((pad, s.L), -1)])
            A = np.concatenate([A, np.ones(pad, dtype=f32)]); IB = np.concatenate([IB, np.zeros(pad, dtype=f32)])
        out = _launch(s, X, what, role=site[1], pair=(A, IB))
        m = I[:out.shape[0]] >= 0
        res[I[:out.shape[0]][m]] = out[m]
        assert (P.canon_bits(out[~m]) == 0).all(), f"{what}: snake(0) != 0 in the padding"
    assert not np.isnan(res).any()
    _SNAKE[key] = res
    return res


def _snake_refs():
    if "refs" not in _SNAKE:
        tab = P.snake_table()
        a, ib = tab.a[tab.grp], tab.ib[tab.grp]
        _SNAKE["refs"] = (P.snake32(tab.x, a, ib), P.snake64(tab.x, a, ib), a, ib)
    return _SNAKE["refs"]


@gpu
@pytest.mark.parametrize("site,name", P.SNAKE_RUNS, ids=[f"{k}-{r}-{n}" for (k, r), n in P.SNAKE_RUNS])
def test_snake_site(site, name):
    tab = P.snake_table()
    y32, y64, a, ib = _snake_refs()
    y = _snake_result(site, name)
    what = f"{site[0]} {site[1]} ({name})"
    poly = np.abs(tab.t) < P.SWITCH
    # figures first: worst |sin^2 error| per bucket of |t| in units of B_SIN, read off the power-of-two rows (ib = 1, |x| <= 2^-12:
    # y - x is sin^2 to within y's own rounding, at most 6e-8)
    pw = tab.kind != P.KINDS.index("generic")
    err = np.abs(y.astype(f64) - y64)
    b = P.bucket_of(tab.t)
    fig = {P.BUCKET_NAMES[i]: float(err[pw & (b == i)].max() / P.B_SIN) for i in range(len(P.BUCKETS))}
    nbad = int((P.canon_bits(y[poly]) != P.canon_bits(y32[poly])).sum())
    nmir = int((P.canon_bits(y[:tab.half]) != P.canon_bits(y[tab.half:])).sum())
    bound = 4 * P.D_REF_SIN2 * np.abs(ib.astype(f64)) + 2.0 ** -24 * np.abs(y64)
    big = float((np.abs(y.astype(f64) - y64) / bound)[~poly].max())
    RESULTS[f"snake {what}"] = dict(sin2_err_over_B_SIN=fig, rows_off_restatement=nbad, rows_off_mirror=nmir, sinf_rows_over_bound=big)
    print(f"{what}: worst |sin^2 error| / B_SIN per bucket {fig}; rows differing from the restatement {nbad} of {int(poly.sum())}, "
          f"from their mirror {nmir}; sinf rows at {big:.3f} of their bound")
    if nbad:
        i = np.nonzero(poly)[0][np.nonzero(P.canon_bits(y[poly]) != P.canon_bits(y32[poly]))[0][:5]]
        print("  first:", [(float(tab.x[j]), float(a[j]), float(ib[j]), float(y[j]), float(y32[j]), P.KINDS[tab.kind[j]]) for j in i])
    assert nbad == 0, f"{what}: {nbad} rows with |t| < 8192 differ from the float32 restatement"
    assert nmir == 0, f"{what}: {nmir} rows differ from their mirrored copy: sin_sq is not even"
    assert big <= 1.0, f"{what}: a sinf row at {big:.3f} of 4 D_REF_SIN2 |ib| + one rounding"


@gpu
def test_snake_sites_agree():
    """every site, every row, the same bits — the sinf rows, which have no restatement, included"""
    ref_key = P.SNAKE_RUNS[0]
    ref = P.canon_bits(_snake_result(*ref_key))
    off = {}
    for site, name in P.SNAKE_RUNS[1:]:
        n = int((P.canon_bits(_snake_result(site, name)) != ref).sum())
        if n:
            off[f"{site[0]} {site[1]} ({name})"] = n
    RESULTS["snake sites off the first"] = off
    assert off == {}, f"rows differing from {ref_key}: {off}"


# ---------------------------------------------------------------- activations
_ACT = {}


def _act_result(site, name, act):
    key = (site, name, act)
    if key not in _ACT:
        s = P.SHAPES[name]
        assert P.KERNEL_OF[s.path & 31] == site[0]
        _ACT[key] = _run_flat(s, P.act_table().v, f"{site[0]} act {act} ({name})", role="act", act=act)
    return _ACT[key]


@gpu
@pytest.mark.parametrize("act", P.ACTS)
@pytest.mark.parametrize("site,name", P.ACT_RUNS, ids=[f"{k}-{n}" for (k, r), n in P.ACT_RUNS])
def test_act_site(site, name, act):
    tab = P.act_table()
    y = _act_result(site, name, act)
    what = f"{site[0]} act {act} ({name})"
    assert not np.isnan(y).any(), f"{what}: NaN"
    if act == 3:
        assert (P.canon_bits(y) == P.canon_bits(np.maximum(tab.v, f32(0)))).all(), f"{what}: ReLU is not exact"
        return
    if act == 5:
        m100 = tab.v == f32(-100.0)
        assert m100.any() and (y[m100] == 0).all(), f"{what}: sigmoid(-100) = {y[m100]!r}"
    fig = P.act_bucket_figures(y, act)
    ratio = {}
    for nm, g, d in zip(tab.names, fig, P.D_REF_ACT[act]):
        ratio[nm] = 0.0 if g == 0 else (float(g / d) if d > 0 else float("inf"))
    worst = max(ratio, key=ratio.get)
    RESULTS[f"act {what}"] = dict(figure=dict(zip(tab.names, fig)), over_D_REF_ACT=ratio)
    print(f"{what}: worst bucket {worst!r} at {ratio[worst]:.3f} D_REF_ACT (bound 4); all: " + ", ".join(f"{k} {v:.2f}" for k, v in ratio.items()))
    bad = {k: v for k, v in ratio.items() if v > 4.0}
    assert bad == {}, f"{what}: buckets beyond 4 D_REF_ACT: {bad}"


@gpu
@pytest.mark.parametrize("act", P.ACTS)
def test_act_sites_agree(act):
    ref = P.canon_bits(_act_result(*P.ACT_RUNS[0], act))
    off = {f"{site[0]} ({name})": int((P.canon_bits(_act_result(site, name, act)) != ref).sum()) for site, name in P.ACT_RUNS[1:]}
    assert not any(off.values()), f"act {act}: values differing from {P.ACT_RUNS[0]}: {off}"


# ---------------------------------------------------------------- snake tables
def _around(v, K):
    out = [f32(v)]
    up = dn = f32(v)
    for _ in range(K):
        up = np.nextafter(up, f32(np.inf)); dn = np.nextafter(dn, f32(-np.inf)); out += [up, dn]
    return out


def _identify(x, y, a0, ib0, K=8):
    """every float32 pair (a, ib) within K ulps of (a0, ib0) whose restatement gives the observed row y bit for bit"""
    found = []
    yb = P.canon_bits(y)
    for a in _around(a0, K):
        s = P.sin_sq32(x * a)
        for ib in _around(ib0, K):
            if (P.canon_bits(x + s * ib) == yb).all():
                found.append((a, ib))
    return found


@gpu
def test_snake_tables_wide_range():
    """launch_snake_tables (snake_raw): alpha, beta in [-6, 6] and beta = -25. Two launches of a 64-channel identity conv with snake on load:
    every alpha beside beta = -25 (1 / b ~ 1e9: y = x + s ib shows s, hence a, at full resolution), and every beta beside alpha = 12
    (x ~ 1e-5 stays below an ulp of s ib, so y shows ib)."""
    al, be = P.table_inputs()
    n = len(al); assert n == len(be) == 64
    a64, ib64 = P.tables64(al, be)
    rng = np.random.default_rng(17)
    w = np.eye(n, dtype=f32).reshape(n, n, 1)
    got_a = np.zeros(n, dtype=f32); got_ib = np.zeros(n, dtype=f32)
    for which in ("a", "ib"):
        if which == "a":
            alr, ber = al, np.full(n, -25.0, dtype=f32)
            u = rng.uniform(1.0, 50.0, (1, 64))
        else:
            alr, ber = np.full(n, 12.0, dtype=f32), be
            u = rng.uniform(0.5, 3.0, (1, 64))
        ar, ibr = P.tables64(alr, ber)
        x = (u / ar[:, None]).astype(f32)
        y, _, _ = q.conv_ex(P.CONV, x, w, snake=(alr, ber), snake_raw=True)
        GPU_RAN.append(1)
        y = y.reshape(n, 64)
        assert np.isfinite(y).all()
        for c in range(n):
            found = _identify(x[c], y[c], f32(ar[c]), f32(ibr[c]))
            assert len(found) == 1, f"channel {c} (alpha {alr[c]}, beta {ber[c]}): {len(found)} float32 pairs within 8 ulps reproduce the row"
            if which == "a":
                got_a[c] = found[0][0]
            else:
                got_ib[c] = found[0][1]
            if which == "a" and c == 0:
                big = found[0][1]
                assert np.isfinite(big) and abs(float(big) / ib64[0] - 1) <= 4 * P.D_REF_TAB_IB, f"1 / b at beta = -25: {big!r}"
    da = float((np.abs(got_a.astype(f64) - a64) / a64).max()); dib = float((np.abs(got_ib.astype(f64) - ib64) / ib64).max())
    RESULTS["snake tables"] = dict(a_rel_dev=da, ib_rel_dev=dib, a_over_D_REF=da / P.D_REF_TAB_A, ib_over_D_REF=dib / P.D_REF_TAB_IB)
    print(f"snake tables: a deviates {da:.3e} = {da / P.D_REF_TAB_A:.2f} D_REF_TAB_A, 1 / b {dib:.3e} = {dib / P.D_REF_TAB_IB:.2f} D_REF_TAB_IB (bound 4)")
    assert da <= 4 * P.D_REF_TAB_A and dib <= 4 * P.D_REF_TAB_IB
