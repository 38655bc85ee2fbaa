"""Tables and references of the pointwise-nonlinearity tests (tests/test_pointwise_reference.py without a GPU,
tests/test_gpu_pointwise_ops.py with one) — TEST INFRASTRUCTURE, no test in here.

What is tested: SnakeBeta (`snake_f` / `sin_sq` of q3_kernels_codec.hip) at each place a conv kernel inlines it, and the epilogue
activations of `conv_act`, over their whole argument range. Every site is observed through an *identity conv*: w = I (a 1 x 1 conv, or
taps that are zero except the current sample's), no bias, a zero residual. In three-plane mode a value v splits exactly into
hi + mid + lo, each is multiplied by 1.0 and added to zeros, and the three-term sum is exact in any order the kernels use; the VALU /
f32-MFMA kernels are fmaf chains onto zero. So y IS the pointwise result, bit for bit (asserted per kernel path before anything else).

The SnakeBeta table. A row is (x, a, ib); the kernel forms t = fl32(x a), s = sin_sq(t), y = fl32(x + fl32(s ib)).
  * power-of-two rows: a = +-2^e, ib = 1, |x| in (2^-15, 2^-12]: t = x a is exact, and y = x + s resolves s to an ulp of y ~ s;
  * generic rows: a = exp(alpha), ib = 1 / (exp(beta) + 1e-9) as a checkpoint would give them, |x| <= min(80, 8 ib): the rounding of
    the product and the two roundings of mul_rn / add_rn (a contracted instance — one fma — differs here, and only here);
  * every row has a mirrored copy with -a (the same x): sin_sq(-t) must give the same bits, so y must.
Targets |t|: random in [2^-20, 8), [8, 64), [64, 512), [512, 4096), [4096, 8192), both signs of x; for EVERY k in 0 .. 2607 the float32
nearest to k pi and to (k + 1/2) pi with both neighbours; +-4 ulps around (k + 1/2) pi for every 7th k (where fl32(t / pi) hits k + 1/2
exactly: rint's ties); 8192 and its two neighbours; [8192, 2^17) for the sinf branch; 0.

References: float64 of the definition with t the float32 product (as the reference implementation scales x in f32), and a float32
restatement of sin_sq / snake_f in numpy whose fma is exact (float64 product — exact for float32 operands — TwoSum, round to odd,
one cast). No denormal appears anywhere in the table (asserted): flushing modes cannot matter."""
import collections
import math

import numpy as np

f32 = np.float32
f64 = np.float64

# ---------------------------------------------------------------- the routine's constants, as written in q3_kernels_codec.hip
INV_PI = f32(0.31830988618379067154)
PI_A = f32(3.140625)
PI_B = f32(9.67502593994140625e-4)
PI_C = f32(1.509957990978376432e-7)
POLY = (f32(-2.50521083854417188e-8), f32(2.75573192239858907e-6), f32(-1.98412698412698413e-4), f32(8.33333333333333333e-3),
        f32(-1.66666666666666667e-1))          # r^11, r^9, r^7, r^5, r^3
SWITCH = f32(8192.0)                             # |t| >= SWITCH: sinf
K_MAX = 2607                                     # the last multiple of pi below 8192 (2607 pi = 8190.13); rint(t / pi) reaches 2608 there

# frozen figures (measured by the functions named; test_pointwise_reference.py re-measures each and holds it to [0.5, 1.0] x the constant)
B_SIN = 3.5e-7           # measure_b_sin(): restatement of sin_sq against float64 over the table, |t| < 8192
D_REF_SIN2 = 1.25e-7     # measure_d_ref_sin2(): numpy float32 sin(t)^2 against float64 over the whole table
D_REF_TAB_A = 1.27e-7    # measure_d_ref_tables(): numpy float32 exp(alpha), relative
D_REF_TAB_IB = 1.3e-7    # ... and 1 / (exp(beta) + 1e-9), relative


# ---------------------------------------------------------------- exact float32 arithmetic in numpy
def fma32(a, b, c):
    """float32 fma(a, b, c), exactly. a b is exact in float64 (24 + 24 bits); TwoSum gives the float64 sum s and its error e;
    where e != 0 the sum is replaced by the neighbour (towards the true value) whose last bit is odd — round to odd — after which
    the cast to float32 rounds once (53 >= 24 + 2 bits). Normal and subnormal float32 results alike; no overflow handling."""
    a, b, c = np.broadcast_arrays(np.asarray(a, dtype=f32), np.asarray(b, dtype=f32), np.asarray(c, dtype=f32))
    p = a.astype(f64) * b.astype(f64)
    c = c.astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)                     # exact: s + e == p + c
    s = np.ascontiguousarray(s)
    even = (s.view(np.int64) & 1) == 0
    nxt = np.nextafter(s, np.where(e > 0, np.inf, -np.inf))
    return np.where((e != 0) & even, nxt, s).astype(f32)


def sin_sq32(t, *, terms=3, pi_b=PI_B, c11=POLY[0], rnd=np.rint):
    """sin_sq() restated: every product and sum rounded once to float32, fmaf exact. Defined for |t| < 8192 (the polynomial branch);
    the keyword arguments are the mutations the reference test applies."""
    t = np.asarray(t, dtype=f32)
    k = rnd(t * INV_PI).astype(f32)
    r = fma32(-k, PI_A, t)
    if terms >= 2:
        r = fma32(-k, pi_b, r)
    if terms >= 3:
        r = fma32(-k, PI_C, r)
    z = r * r
    p = fma32(z, c11, POLY[1])
    p = fma32(z, p, POLY[2])
    p = fma32(z, p, POLY[3])
    p = fma32(z, p, POLY[4])
    s = fma32(r * z, p, r)
    return s * s


def snake32(x, a, ib, contracted=False, **mut):
    """snake_f restated: t = fl(x a), y = fl(x + fl(s ib)); contracted: y = fma(s, ib, x), what a contracting compiler would make of it"""
    x = np.asarray(x, dtype=f32); a = np.asarray(a, dtype=f32); ib = np.asarray(ib, dtype=f32)
    s = sin_sq32(x * a, **mut)
    return fma32(s, ib, x) if contracted else x + s * ib


def sin2_64(t):
    return np.sin(np.asarray(t, dtype=f32).astype(f64)) ** 2


def snake64(x, a, ib):
    """the float64 definition: x + sin(t)^2 ib with t the float32 product"""
    x = np.asarray(x, dtype=f32); a = np.asarray(a, dtype=f32); ib = np.asarray(ib, dtype=f32)
    return x.astype(f64) + sin2_64(x * a) * ib.astype(f64)


def canon_bits(v):
    """bit patterns with -0 mapped to +0"""
    u = np.ascontiguousarray(v, dtype=f32).view(np.uint32).copy()
    u[u == 0x80000000] = 0
    return u


# ---------------------------------------------------------------- the SnakeBeta table
POW2_E = tuple(range(-9, 33, 3))          # a = 2^e; a target |t| = m 2^ex (m in [0.5, 1)) goes to the smallest e >= ex + 12
GENERIC = ((-1.7, -3.0), (-0.4, 0.6), (0.3, -0.9), (1.1, 2.0), (2.3, -6.0), (4.0, 5.0), (3.0, -2.0))       # (alpha, beta) of the generic rows
N_GENERIC = 1024
BUCKETS = ((0.0, 8.0), (8.0, 64.0), (64.0, 512.0), (512.0, 4096.0), (4096.0, 8192.0), (8192.0, 131072.0))       # by |t|
BUCKET_NAMES = ("[0,8)", "[8,64)", "[64,512)", "[512,4096)", "[4096,8192)", "[8192,2^17)")

SnakeTable = collections.namedtuple("SnakeTable", "x grp a ib t kind half")
# x [N], grp [N] group of a row; a, ib [G] per group; t [N] = fl32(x a[grp]); kind [N] (index into KINDS); half = N / 2: row i + half
# is the mirrored copy (-a) of row i
KINDS = ("random", "kpi", "halfpi", "tie", "switch", "sinf", "zero", "generic")


def _near(v64):
    """float32 nearest to each v and both neighbours, flat"""
    c = np.asarray(v64, dtype=f64).astype(f32)
    return np.concatenate([np.nextafter(c, f32(0)), c, np.nextafter(c, f32(np.inf))])


def _targets():
    """positive targets |t| (float32) with their kind; the signs come with x"""
    rng = np.random.default_rng(20250611)
    out = []
    out.append((np.exp2(rng.uniform(-20.0, 3.0, 3000)).astype(f32), "random"))
    for lo, hi in BUCKETS[1:5]:
        out.append((rng.uniform(lo, hi, 3000).astype(f32), "random"))
    k = np.arange(1, K_MAX + 1, dtype=f64)
    out.append((_near(k * math.pi), "kpi"))
    k = np.arange(0, K_MAX + 1, dtype=f64)
    out.append((_near((k + 0.5) * math.pi), "halfpi"))
    c = ((np.arange(0, K_MAX + 1, 7, dtype=f64) + 0.5) * math.pi).astype(f32)
    around = [c]
    up, dn = c, c
    for _ in range(4):
        up = np.nextafter(up, f32(np.inf)); dn = np.nextafter(dn, f32(0)); around += [up, dn]
    out.append((np.concatenate(around), "tie"))
    out.append((np.array([np.nextafter(SWITCH, f32(0)), SWITCH, np.nextafter(SWITCH, f32(np.inf))], dtype=f32), "switch"))
    big = [rng.uniform(8192.0, 131072.0, 3000).astype(f32), _near(np.arange(2608, 41700, 97, dtype=f64) * math.pi),
           _near((np.arange(2608, 41700, 89, dtype=f64) + 0.5) * math.pi)]
    out.append((np.concatenate(big), "sinf"))
    out.append((np.zeros(1, dtype=f32), "zero"))
    t = np.concatenate([o[0] for o in out])
    kind = np.concatenate([np.full(len(o[0]), KINDS.index(o[1])) for o in out])
    assert (t >= 0).all() and (t < 131072.0).all() and ((t == 0) | (t >= 2.0 ** -20)).all()
    return t, kind, rng


_TABLE = None


def snake_table():
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    t, kind, rng = _targets()
    # power-of-two rows: x = t 2^-e, exact
    _, ex = np.frexp(t)
    ex = np.where(t == 0, -30, ex)
    gi = np.searchsorted(np.array(POW2_E), ex + 12)                  # smallest e >= ex + 12
    assert gi.max() < len(POW2_E)
    e = np.array(POW2_E)[gi]
    x = np.ldexp(t, -e).astype(f32)
    assert (np.ldexp(x.astype(f64), e) == t.astype(f64)).all() and (np.abs(x) <= 2.0 ** -12).all()
    x = np.where(rng.integers(0, 2, len(x)) == 1, -x, x).astype(f32)          # both signs of t
    a = [f32(2.0 ** ee) for ee in POW2_E]
    ib = [f32(1.0)] * len(POW2_E)
    xs, gs, ks = [x], [gi], [kind]
    for j, (al, be) in enumerate(GENERIC):
        aj = f32(math.exp(al)); ibj = f32(1.0 / (math.exp(be) + 1e-9))
        a.append(aj); ib.append(ibj)
        xg = (rng.uniform(-1.0, 1.0, N_GENERIC) * min(80.0, 8.0 * float(ibj))).astype(f32)      # activation scale, but x and s ib within 2^4: both roundings show
        xs.append(xg); gs.append(np.full(N_GENERIC, len(POW2_E) + j)); ks.append(np.full(N_GENERIC, KINDS.index("generic")))
    x = np.concatenate(xs); g = np.concatenate(gs); kd = np.concatenate(ks)
    G = len(a)
    a = np.array(a + [-v for v in a], dtype=f32); ib = np.array(ib + ib, dtype=f32)
    x = np.concatenate([x, x]); g = np.concatenate([g, g + G]); kd = np.concatenate([kd, kd])
    tt = (x * a[g]).astype(f32)
    half = len(x) // 2
    assert (tt[half:] == -tt[:half]).all()
    pw = kd != KINDS.index("generic")
    assert (np.abs(tt[:half][pw[:half]]) == t).all()          # the power-of-two rows hit their targets exactly
    assert (np.abs(tt[~pw]) < 8192.0).all()
    tiny = np.finfo(f32).tiny
    assert ((x == 0) | (np.abs(x) >= tiny * 2.0 ** 30)).all() and np.isfinite(tt).all()
    _TABLE = SnakeTable(x, g, a, ib, tt, kd, half)
    return _TABLE


def bucket_of(t):
    """index into BUCKETS by |t|"""
    at = np.abs(np.asarray(t, dtype=f64))
    return np.searchsorted(np.array([b[1] for b in BUCKETS]), at, side="right")


def pack(tab_x, tab_grp, a, ib, C, L):
    """The table laid out for launches of C channels x L columns: a channel holds L rows of ONE group (its a / ib). ->
    list of (x [C][L], a [C], ib [C], idx [C][L]) with idx the table row of a cell, -1 for padding (x = 0; spare channels a = 1, ib = 0)."""
    chunks = []
    for g in range(len(a)):
        rows = np.nonzero(tab_grp == g)[0]
        for i in range(0, len(rows), L):
            chunks.append((g, rows[i:i + L]))
    out = []
    for i in range(0, len(chunks), C):
        X = np.zeros((C, L), dtype=f32); A = np.ones(C, dtype=f32); IB = np.zeros(C, dtype=f32); I = np.full((C, L), -1, dtype=np.int64)
        for c, (g, rows) in enumerate(chunks[i:i + C]):
            X[c, :len(rows)] = tab_x[rows]; I[c, :len(rows)] = rows; A[c] = a[g]; IB[c] = ib[g]
        out.append((X, A, IB, I))
    return out


def pack_flat(v, C, L):
    """a flat table without per-channel operands over launches of C x L -> list of (x [C][L], idx [C][L])"""
    n = C * L
    out = []
    for i in range(0, len(v), n):
        X = np.zeros(n, dtype=f32); I = np.full(n, -1, dtype=np.int64)
        m = min(n, len(v) - i)
        X[:m] = v[i:i + m]; I[:m] = np.arange(i, i + m)
        out.append((X.reshape(C, L), I.reshape(C, L)))
    return out


# ---------------------------------------------------------------- the call sites and the shapes that reach them
# ConvPath codes (include/q3tts.h), as tests/test_gpu_conv_ops.py names them
OUT1, OUT1_V4, SMALL4, G64x64, MFMA64, VALU, UNIT3 = 1, 2, 3, 9, 12, 14, 15
SEG, CIS128 = 64, 128
CONV, UNIT = 0, 2

Shape = collections.namedtuple("Shape", "name path kind C L k packed")
# the smallest shape per kernel from the path rules test_gpu_conv_ops.py documents; C = cin = cout (the out1 kernels: cin, cout = 1)
SHAPES = collections.OrderedDict((s.name, s) for s in (
    Shape("valu", VALU, CONV, 16, 2048, 1, False),                     # unpacked, cout < 32
    Shape("mfma", MFMA64, CONV, 64, 512, 1, False),                    # unpacked, cout % 64 == 0
    Shape("x3", G64x64, CONV, 64, 512, 1, True),                       # packed, cin < 256: 32-channel stages
    Shape("x3_cis128", G64x64 | CIS128, CONV, 256, 128, 1, True),      # packed, k = 1, cin >= 256: 128-channel stages
    Shape("small", SMALL4 | SEG, CONV, 512, 32, 1, True),              # k_lin_small: cin = cout = 512, L <= 32
    Shape("out1", OUT1, CONV, 16, 8192, 1, False),                     # cout = 1
    Shape("out1_v4", OUT1_V4, CONV, 16, 8192, 7, False),               # cout = 1, k = 7, L % 4 == 0
    Shape("unit", UNIT3, UNIT, 96, 4096, 7, True),                     # the fused residual unit
))

# every place q3_kernels_codec.hip inlines snake_f (twelve: six on load, five on the output, one between the unit's convs) and
# conv_act (four), by kernel template and role -> the shapes that run it. Kept by hand: a new call site needs a row here.
SNAKE_SITES = collections.OrderedDict((
    (("k_conv1d", "load"), ("valu",)), (("k_conv1d_mfma", "load"), ("mfma",)), (("k_conv_bf16x3", "load"), ("x3", "x3_cis128")),
    (("k_lin_small_bf16x3", "load"), ("small",)), (("k_conv_out1", "load"), ("out1",)), (("k_conv_out1_v4", "load"), ("out1_v4",)),
    (("k_conv1d", "post"), ("valu",)), (("k_conv1d_mfma", "post"), ("mfma",)), (("k_conv_bf16x3", "post"), ("x3", "x3_cis128")),
    (("k_lin_small_bf16x3", "post"), ("small",)), (("k_resunit_bf16x3", "post"), ("unit",)),
    (("k_resunit_bf16x3", "mid"), ("unit",)),
))
ACT_SITES = collections.OrderedDict((
    (("k_conv1d", "act"), ("valu",)), (("k_conv1d_mfma", "act"), ("mfma",)), (("k_conv_bf16x3", "act"), ("x3", "x3_cis128")),
    (("k_lin_small_bf16x3", "act"), ("small",)),
))
# the kernel template behind a path code's low five bits
KERNEL_OF = {OUT1: "k_conv_out1", OUT1_V4: "k_conv_out1_v4", SMALL4: "k_lin_small_bf16x3", G64x64: "k_conv_bf16x3", MFMA64: "k_conv1d_mfma",
             VALU: "k_conv1d", UNIT3: "k_resunit_bf16x3"}
SNAKE_RUNS = [(site, sh) for site, shapes in SNAKE_SITES.items() for sh in shapes]          # (site, shape name): one table pass each
ACT_RUNS = [(site, sh) for site, shapes in ACT_SITES.items() for sh in shapes]


def identity_w(s):
    """the identity conv's weights: [cout][cin][k], the only non-zero tap the current sample's (kk = k - 1); the out1 kernels observe
    channel 0"""
    cout = 1 if s.name.startswith("out1") else s.C
    w = np.zeros((cout, s.C, s.k), dtype=f32)
    for o in range(cout):
        w[o, o, s.k - 1] = 1.0
    return w


def channel_table():
    """x for the exactness check of the channel itself: full 24-bit mantissas over exponents 2^-60 .. 2^100 (the lo plane stays normal,
    the hi plane finite), both signs, +-0, and values whose planes round up into the next binade"""
    rng = np.random.default_rng(7)
    n = 16384
    m = (rng.integers(1 << 23, 1 << 24, n) | 1).astype(f64)
    v = np.ldexp(m, rng.integers(-60, 100, n) - 23) * rng.choice([-1.0, 1.0], n)
    edge = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** 100, -2.0 ** 100, 2.0 ** -60] +
                    [float.fromhex(h) for h in ("0x1.fffffep0", "0x1.ff7ffep0", "0x1.ff8000p0", "0x1.007f80p0", "0x1.ffffp99")])
    v = np.concatenate([edge, v]).astype(f32)
    assert np.isfinite(v).all() and (np.abs(v) <= 2.0 ** 100).all()
    return v


# ---------------------------------------------------------------- activations
ACTS = (1, 3, 4, 5, 6)                    # GELU-erf, ReLU, tanh(ReLU), sigmoid, ELU
_erf = np.frompyfunc(math.erf, 1, 1)


def act64(v, act):
    """float64 of the formulas as conv_act writes them"""
    v = np.asarray(v, dtype=f32).astype(f64)
    if act == 1:
        return 0.5 * v * (1.0 + _erf(v * f64(f32(0.70710678118654752440))).astype(f64))
    if act == 3:
        return np.maximum(v, 0.0)
    if act == 4:
        return np.tanh(np.maximum(v, 0.0))
    if act == 5:
        with np.errstate(over="ignore"):
            return 1.0 / (np.exp(-v) + 1.0)
    if act == 6:
        return np.where(v > 0, v, np.exp(np.minimum(v, 0.0)) - 1.0)
    raise ValueError(act)


def act32(v, act):
    """the same formulas in numpy float32 (erf: float64 rounded to float32, a correctly rounded erff)"""
    v = np.asarray(v, dtype=f32)
    with np.errstate(over="ignore", under="ignore"):
        if act == 1:
            e = _erf((v * f32(0.70710678118654752440)).astype(f64)).astype(f64).astype(f32)
            return f32(0.5) * v * (f32(1.0) + e)
        if act == 3:
            return np.maximum(v, f32(0))
        if act == 4:
            return np.tanh(np.maximum(v, f32(0)))
        if act == 5:
            return f32(1.0) / (np.exp(-v) + f32(1.0))
        if act == 6:
            return np.where(v > 0, v, np.exp(np.minimum(v, f32(0))) - f32(1.0)).astype(f32)
    raise ValueError(act)


ActTable = collections.namedtuple("ActTable", "v bucket names")
_ACT_TABLE = None


def act_table():
    """v [N], bucket [N], bucket names. Each bucket spans at most a factor of 8 in |v| and one sign."""
    global _ACT_TABLE
    if _ACT_TABLE is not None:
        return _ACT_TABLE
    rng = np.random.default_rng(11)
    vs, bs, names = [], [], []

    def add(name, vals):
        names.append(name); vs.append(np.asarray(vals, dtype=f32)); bs.append(np.full(len(vals), len(names) - 1))
    add("zero", [0.0, -0.0])
    for sg, sn in ((1.0, "+"), (-1.0, "-")):
        for j in range(9):                                               # 2^-20 .. 100 in factors of 8
            lo, hi = 2.0 ** (3 * j - 20), min(2.0 ** (3 * j - 17), 100.0)
            u = np.exp2(rng.uniform(math.log2(lo), math.log2(hi), 400))
            add(f"{sn}[2^{3 * j - 20},{'100' if hi == 100.0 else f'2^{3 * j - 17}'}]", sg * np.concatenate([[lo, hi], u]))
        add(f"{sn}[5,10] dense", sg * np.linspace(5.0, 10.0, 2001))      # erff / tanhf saturation
        add(f"{sn}[85,92]", sg * np.concatenate([np.linspace(85.0, 92.0, 701), [88.7, 88.72283905206835, 88.73, 87.33654475055310898657]]))
        add(f"{sn}[100,108]", sg * np.concatenate([np.linspace(100.0, 108.0, 401), [103.9720840454, 104.0]]))      # 104 ~ ln(2^150)
    for j, (lo, hi) in enumerate(((1e-6, 8e-6), (8e-6, 6.4e-5), (6.4e-5, 5.12e-4), (5.12e-4, 1e-3))):
        add(f"-[{lo:g},{hi:g}] elu", -np.concatenate([[lo, hi], np.exp(rng.uniform(math.log(lo), math.log(hi), 400))]))
    v = np.concatenate(vs); b = np.concatenate(bs)
    assert np.isfinite(v).all() and (np.abs(v) <= 108.0).all()
    _ACT_TABLE = ActTable(v, b, tuple(names))
    return _ACT_TABLE


def act_bucket_figures(y, act):
    """per bucket: max |y - y64| / max |y64| (0 where y is exact, inf where y64 is all zero and y is not)"""
    tab = act_table()
    ref = act64(tab.v, act)
    err = np.abs(np.asarray(y, dtype=f32).astype(f64) - ref)
    out = []
    for b in range(len(tab.names)):
        m = tab.bucket == b
        e, r = err[m].max(), np.abs(ref[m]).max()
        out.append(0.0 if e == 0 else (e / r if r > 0 else math.inf))
    return out


def measure_d_ref_act():
    """{act: [per bucket figure of numpy float32]}"""
    return {act: act_bucket_figures(act32(act_table().v, act), act) for act in ACTS if act != 3}


# D_REF_ACT[act][bucket]: measure_d_ref_act() frozen (at most 1.2 x above the measurement; 0 where numpy float32 is exact)
D_REF_ACT = {
    1: (0.0, 7.182e-08, 8.108e-08, 7.053e-08, 7.620e-08, 1.081e-07, 1.017e-07, 6.632e-08, 2.537e-08, 0.0, 4.920e-08, 0.0, 0.0, 5.772e-08, 5.241e-08,
        5.809e-08, 5.622e-08, 5.769e-08, 8.954e-08, 2.441e-07, 1.758e-06, 0.0, 6.335e-02, 0.0, 0.0, 7.039e-08, 6.295e-08, 8.752e-08, 7.086e-08),
    4: (0.0, 2.134e-11, 1.366e-09, 4.495e-08, 4.991e-08, 5.034e-08, 6.448e-08, 6.782e-08, 6.203e-08, 2.784e-14, 6.466e-08, 0.0, 0.0, 0.0, 0.0,
        0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    5: (0.0, 1.082e-07, 1.072e-07, 1.311e-07, 1.393e-07, 1.443e-07, 1.100e-07, 8.604e-08, 9.334e-08, 6.084e-08, 9.658e-08, 0.0, 0.0, 1.432e-07, 1.456e-07,
        1.485e-07, 1.386e-07, 1.501e-07, 1.424e-07, 1.575e-07, 1.124e-07, 7.739e-08, 1.217e-07, 2.658e-02, 1.1, 1.426e-07, 1.405e-07, 1.510e-07, 1.478e-07),
    6: (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.230e-02, 1.487e-03, 2.408e-04, 3.021e-05, 3.915e-06, 4.725e-07,
        1.329e-07, 3.755e-08, 2.947e-08, 3.289e-08, 0.0, 0.0, 1.149e-02, 1.457e-03, 2.334e-04, 1.134e-04),
}


# ---------------------------------------------------------------- measurements behind the frozen figures
def measure_b_sin():
    tab = snake_table()
    m = np.abs(tab.t) < SWITCH
    return float(np.abs(sin_sq32(tab.t[m]).astype(f64) - sin2_64(tab.t[m])).max())


def measure_d_ref_sin2():
    tab = snake_table()
    s = np.sin(tab.t)
    assert s.dtype == f32
    return float(np.abs((s * s).astype(f64) - sin2_64(tab.t)).max())


# snake tables: alpha, beta over [-6, 6] and beta = -25 (there 1e-9 dominates: 1 / b ~ 1e9, finite)
def table_inputs():
    rng = np.random.default_rng(13)
    al = np.concatenate([[-6.0, 6.0, 0.0], rng.uniform(-6.0, 6.0, 61)]).astype(f32)
    be = np.concatenate([[-25.0, -6.0, 6.0, 0.0], rng.uniform(-6.0, 6.0, 60)]).astype(f32)
    return al, be


def tables64(al, be):
    return np.exp(al.astype(f64)), 1.0 / (np.exp(be.astype(f64)) + 1e-9)


def tables32(al, be):
    """numpy float32 of k_snake_tables' expressions"""
    return np.exp(al), f32(1.0) / (np.exp(be) + f32(1e-9))


def measure_d_ref_tables():
    al, be = table_inputs()
    a64, ib64 = tables64(al, be)
    a32, ib32 = tables32(al, be)
    assert a32.dtype == f32 and ib32.dtype == f32
    return float((np.abs(a32.astype(f64) - a64) / a64).max()), float((np.abs(ib32.astype(f64) - ib64) / ib64).max())
