"""Inputs and references of the op-level sampler tests (k_sample through q3_sample_ex). No GPU, no library: numpy only.

The reference is a restatement of SURVEY.md Appendix C (sampling.rs:140-319, lib.rs:1271-1322), written twice — float32 with sequential
sums (np.cumsum in float32; never np.sum, which sums pairwise) and float64. The VALUE pipeline (penalty product, suppression, EOS mask,
temperature product, the top-k threshold) is float32 in both: those are single correctly rounded operations and exact comparisons, so
they have one right answer. Only what is summed — the two softmaxes and the two running sums — exists in two precisions.

Decisions by construction. expf differs by ulps between ocml and numpy, so a `top_p` next to a cumulative sum or a `u` next to a cdf step
has no single right answer. build() therefore works backwards: it picks the cut and the target id first, then sets top_p to the midpoint
between the two cumulative sums around the cut and u to the midpoint of the target's cdf interval, both in float64, and asserts that the
float32 values the kernel receives are at least tol = max(4 * max|sum32 - sum64|, 2^-22) of that row away from the nearest step ("four
times what numpy float32 deviates"). For such a row the expected id is exact. Rows whose decisive quantities are exactly
representable (equal logits: e = 1 under any expf; n = 2, 4 entries: 1/n and its multiples exact) are marked `exact` and say why.

Fuzz rows use a random u over random option sets; a row is AMBIGUOUS when top_p lies within tol of a cumulative sum or u within tol of a
cdf step, and then may match any id between the two neighbours. At most 5 % of a case's rows may be ambiguous (FUZZ_CAP)."""
from dataclasses import dataclass, field, replace
from typing import Optional

import numpy as np

F32 = np.float32
SEL_MAX = 1024            # k_sample: largest survivor set the radix select orders itself; beyond it the bitonic sort runs
WAVE = 64                 # k_sample: sequential sums of up to 64 entries are done by one wave, more by one thread
FUZZ_CAP = 0.05
NEG_INF = F32(-np.inf)


# ------------------------------------------------------------------------------------------------------------------ options
@dataclass(frozen=True)
class Opt:
    """the fields of SynthesisOptions the sampler reads (eos None = no EOS id)"""
    temperature: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    rep: float = 1.0
    eos: Optional[int] = None
    min_new: int = 0


def host_row(o: Opt) -> dict:
    """the per-row record a session derives from a request's options (sample_row; sampling.rs:140-319 branch conditions)"""
    with np.errstate(divide="ignore"):
        rep_inv = F32(1.0) / F32(o.rep)
        inv_temp = F32(np.float64(1.0) / np.float64(o.temperature))
    return dict(inv_temp=inv_temp, apply_temp=int(o.temperature != 1.0 and o.temperature > 0.0), greedy=int(o.temperature < 0.01),
                top_k=int(o.top_k), top_p=F32(o.top_p), use_top_p=int(0.0 < o.top_p < 1.0),
                rep_pen=F32(o.rep), rep_inv=rep_inv, use_rep=int(o.rep != 1.0 and not abs(o.rep - 1.0) < 1e-9),
                eos_id=-1 if o.eos is None else int(o.eos), min_new_tokens=int(o.min_new))


# ------------------------------------------------------------------------------------------------------------------ reference
MUTANTS = ("topk_gt", "topp_ge", "tie_desc_index", "topp_unfiltered", "final_sorted", "suppress_1023", "zero_div", "eos_le", "cdf_gt")


def _first_max(v):
    """first maximum, NaN never wins, 0 when nothing compares (block_argmax_first)"""
    w = np.where(np.isnan(v), NEG_INF, v)
    return int(np.argmax(w))


def values(logits, r, seen=None, tc=0, codec_eos=2150, suppress=True, mutant=None):
    """steps 1-4: the float32 row the selection works on"""
    v = np.array(logits, dtype=F32)
    V = v.size
    with np.errstate(invalid="ignore", over="ignore"):
        if r["use_rep"] and seen is not None:
            m = np.asarray(seen) != 0
            pos = (v >= 0) if mutant == "zero_div" else (v > 0)             # v > 0 ? v / rep : v * rep — a zero logit is MULTIPLIED
            v = np.where(m, np.where(pos, v * r["rep_inv"], v * r["rep_pen"]), v).astype(F32)
        if suppress:
            lo = V - (1023 if mutant == "suppress_1023" else 1024)
            idx = np.arange(V)
            v[(idx >= lo) & (idx != codec_eos)] = NEG_INF
        masked = tc <= r["min_new_tokens"] if mutant == "eos_le" else tc < r["min_new_tokens"]
        if masked and 0 <= r["eos_id"] < V:
            v[r["eos_id"]] = NEG_INF
        if r["apply_temp"]:
            v = ((v * r["inv_temp"]).astype(F32) + F32(0.0)).astype(F32)
    return v


@dataclass
class Ref:
    id: int
    n_keep: int = 0
    cut: int = 0
    tie: int = 0
    order: Optional[np.ndarray] = None        # kept indices, sorted (value descending, index ascending)
    cum: Optional[np.ndarray] = None          # running top-p probability over `order` (None: top-p off)
    ids: Optional[np.ndarray] = None          # the `cut` survivors in index order
    cdf: Optional[np.ndarray] = None          # running probability over `ids`


def _seq_softmax_cumsum(x, mx, dt):
    with np.errstate(invalid="ignore"):
        e = np.exp(x.astype(dt) - dt(mx))
    s = np.cumsum(e, dtype=dt)[-1]
    pr = (e / s).astype(dt)
    return np.cumsum(pr, dtype=dt)


def sample_ref(logits, u, r, seen=None, tc=0, codec_eos=2150, suppress=True, dt=F32, mutant=None, force_cut=None) -> Ref:
    """the whole sampler on one row; dt = float32 (sequential, the kernel's arithmetic) or float64. force_cut: take this cut instead of
    comparing with top_p (ambiguity analysis)."""
    v = values(logits, r, seen, tc, codec_eos, suppress, mutant)
    V = v.size
    if r["greedy"]:
        return Ref(_first_max(v))
    idx = np.arange(V)
    thr, tie = None, 0
    if r["top_k"] > 0:
        thr = np.sort(v)[::-1][min(r["top_k"], V) - 1]
        keep = (v > thr) if mutant == "topk_gt" else (v >= thr)
        tie = int((v == thr).sum())
    else:
        keep = np.ones(V, bool)
    kept = idx[keep]
    n_keep = kept.size
    if n_keep == 0:
        return Ref(0, 0, 0, tie)
    kv = v[kept]
    second = -kept if mutant == "tie_desc_index" else kept
    order = kept[np.lexsort((second, -kv))]           # -(+0) and -(-0) compare equal: the index decides, as in sort_before
    mx = v[order[0]]
    cut, cum = n_keep, None
    if r["use_top_p"]:
        if mutant == "topp_unfiltered":
            full = idx[np.lexsort((idx, -v))]
            cum = _seq_softmax_cumsum(v[full], mx, dt)
        else:
            cum = _seq_softmax_cumsum(v[order], mx, dt)
        tp = dt(r["top_p"])
        over = (cum >= tp) if mutant == "topp_ge" else (cum > tp)
        if over.any():
            cut = min(int(np.argmax(over)) + 1, n_keep)
    if force_cut is not None:
        cut = force_cut
    ids = order[:cut] if mutant == "final_sorted" else np.sort(order[:cut])
    cdf = _seq_softmax_cumsum(v[ids], mx, dt)
    pick = 0
    uu = dt(F32(u))
    if uu > 0:
        hit = (cdf > uu) if mutant == "cdf_gt" else (cdf >= uu)
        if hit.any():
            pick = int(ids[int(np.argmax(hit))])
    return Ref(pick, n_keep, cut, tie, order, cum, ids, cdf)


def predict_path(n_keep, cut, tie, top_k, V):
    """which way k_sample goes for a sampled (non-greedy) row: (selection, top-p sums, final sums). The radix select orders the survivors
    itself while there are at most SEL_MAX of them — n_keep = (entries above the threshold) + tie, so only a tie set can push a top-k
    below SEL_MAX over it; the sums of up to WAVE entries are done by one wave."""
    assert cut <= n_keep and tie <= n_keep
    select = "radix" if 0 < top_k < V and n_keep <= SEL_MAX else "bitonic"
    return (select, "wave" if n_keep <= WAVE else "thread", "wave" if cut <= WAVE else "thread")


ALL_PATHS = {(s, p, f) for s in ("radix", "bitonic") for (p, f) in (("wave", "wave"), ("thread", "wave"), ("thread", "thread"))}


def tol_of(a32, a64):
    return max(4.0 * float(np.max(np.abs(a32.astype(np.float64) - a64))), 2.0 ** -22)


# ------------------------------------------------------------------------------------------------------------------ rows
@dataclass
class Row:
    name: str
    logits: np.ndarray
    opt: Opt
    u: float
    expect: int
    seen: Optional[np.ndarray] = None
    tc: int = 0
    codec_eos: int = 2150
    suppress: bool = False
    allowed: frozenset = frozenset()          # fuzz rows: every id the tolerance admits (expect included)
    exact: str = ""                           # why the row needs no margin (exactly representable decision)
    path: tuple = ()
    margin: float = np.inf                    # smallest (distance to a step) / tol of the row's decisions
    n_keep: int = 0
    cut: int = 0
    tie: int = 0

    @property
    def V(self):
        return self.logits.size

    def ref(self, dt=F32, mutant=None):
        return sample_ref(self.logits, self.u, host_row(self.opt), self.seen, self.tc, self.codec_eos, self.suppress, dt, mutant)


def _finish(row: Row, check_p: bool, check_u: bool) -> Row:
    """fill in expectation, path and margins; assert the construction rule"""
    r32, r64 = row.ref(F32), row.ref(np.float64)
    assert r32.id == row.expect, (row.name, r32.id, row.expect)
    assert row.exact or r64.id == row.expect, (row.name, r64.id, row.expect)       # an `exact` row is decided by float32 arithmetic itself
    row.n_keep, row.cut, row.tie = r64.n_keep, r64.cut, r64.tie
    h = host_row(row.opt)
    if h["greedy"]:
        row.path = ("greedy",)
        return row
    assert (row.exact or r32.cut == r64.cut) and r32.n_keep == r64.n_keep, row.name
    row.path = predict_path(r64.n_keep, r64.cut, r64.tie, h["top_k"], row.V)
    if h["use_top_p"] and check_p:
        t = tol_of(r32.cum, r64.cum)
        d = float(np.min(np.abs(r64.cum - float(h["top_p"]))))
        assert d >= t, f"{row.name}: top_p {d:.3e} from a cumulative sum, tolerance {t:.3e}"
        row.margin = min(row.margin, d / t)
    if check_u:
        t = tol_of(r32.cdf, r64.cdf)
        d = float(np.min(np.abs(r64.cdf - float(F32(row.u)))))
        assert d >= t, f"{row.name}: u {d:.3e} from a cdf step, tolerance {t:.3e}"
        row.margin = min(row.margin, d / t)
    return row


def build(name, logits, opt: Opt, *, cut=None, targets=("first", "mid", "last"), seen=None, tc=0, codec_eos=2150, suppress=False):
    """constructed rows of one base row: `cut` (int, or "n_keep") fixes top_p by working backwards, each target fixes a u. Targets name a
    survivor in index order ("first", "mid", "last"), "edge" = the last entry inside the cut in SORTED order, or an int position."""
    logits = np.asarray(logits, dtype=F32)
    h = host_row(opt)
    assert not h["greedy"]
    if cut is not None:
        probe = replace(opt, top_p=0.5)
        r = sample_ref(logits, 0.5, host_row(probe), seen, tc, codec_eos, suppress, np.float64)
        c = r.n_keep if cut == "n_keep" else cut
        assert 1 <= c <= r.n_keep, (name, c, r.n_keep)
        lo = 0.0 if c == 1 else float(r.cum[c - 2])
        hi = 1.0 if c == r.n_keep else float(r.cum[c - 1])       # cut = n_keep whether the last sum exceeds top_p or none does
        opt = replace(opt, top_p=float(F32(0.5 * (lo + hi))))
        assert 0.0 < opt.top_p < 1.0, name
    r = sample_ref(logits, 0.5, host_row(opt), seen, tc, codec_eos, suppress, np.float64)
    assert cut is None or r.cut == (r.n_keep if cut == "n_keep" else cut), (name, r.cut, cut)
    rows = []
    for t in targets:
        n = r.ids.size
        if t == "edge":
            k = int(np.searchsorted(r.ids, r.order[r.cut - 1]))
        else:
            k = {"first": 0, "mid": n // 2, "last": n - 1}.get(t, t)
        lo = 0.0 if k == 0 else float(r.cdf[k - 1])
        hi = 1.0 if k == n - 1 else float(r.cdf[k])
        u = float(F32(0.5 * (lo + hi)))
        rows.append(_finish(Row(f"{name}/{t}", logits, opt, u, int(r.ids[k]), seen, tc, codec_eos, suppress), True, True))
    return rows


def fixed(name, logits, opt: Opt, u, expect, *, exact="", seen=None, tc=0, codec_eos=2150, suppress=False, check_p=True):
    """one row with a given u (and top_p): margins are asserted unless `exact` says why the decision is exactly representable"""
    row = Row(name, np.asarray(logits, dtype=F32), opt, float(u), int(expect), seen, tc, codec_eos, suppress, exact=exact)
    return [_finish(row, check_p and not exact, not exact)]


def gauss(seed, V, scale=1.0, shift=0.0):
    return (scale * np.random.default_rng(seed).standard_normal(V) + shift).astype(F32)


def _seen(V, *idx):
    s = np.zeros(V, np.uint8); s[list(idx)] = 1
    return s


SIZES_V = (2, 3, 63, 64, 65, 1000, 1024, 1025, 2048, 3072, 4095, 4096)


def _size_rows():
    rows = []
    for V in SIZES_V:
        ks = sorted({k for k in (0, 1, 2, 50, 63, 64, 65, V - 1, V, V + 5) if k >= 0})
        for j, k in enumerate(ks):
            n_keep = V if k == 0 or k >= V else k
            lg = gauss(1000 * V + k, V, 1.0 if n_keep <= 65 else 0.3)
            cut = None if n_keep == 1 or j % 3 == 0 else max(1, (2 * n_keep) // 3)       # every third row without top-p
            tg = ("first",) if V == 2 or n_keep == 1 or cut == 1 else ("first", "mid", "last")
            rows += build(f"size/V{V}/k{k}", lg, Opt(top_k=k), cut=cut, targets=tg)
    return rows


def _tie_rows():
    rows = []
    # 100 equal values straddling k = 50 (30 above them)
    lg = gauss(1, 1000, 0.5, -3.0); p = np.random.default_rng(2).permutation(1000)
    lg[p[:30]] = F32(1.5) + F32(0.01) * np.arange(30, dtype=F32); lg[p[30:130]] = F32(1.0)
    rows += build("tie/100_at_k50", lg, Opt(top_k=50), cut=90, targets=("first", "mid", "last", "edge"))
    # a survivor set of exactly SEL_MAX (last radix row) and SEL_MAX + 1 (first fallback row): 10 above, 1014 / 1015 equal
    lg = gauss(3, 1100, 0.3, -4.0); p = np.sort(np.random.default_rng(4).permutation(1100)[:1025])
    lg[p[:10]] = F32(0.5); lg[p[10:1024]] = F32(0.0)
    for n in (1024, 1025):
        g = lg.copy()
        if n == 1025:
            g[p[1024]] = F32(0.0)
        rr = build(f"tie/nsel{n}", g, Opt(top_k=50), targets=("first", "mid", 1000))
        assert all(x.n_keep == n for x in rr)
        rows += rr
    # an all-equal row, below and above SEL_MAX
    for V in (1000, 1100):
        rows += build(f"tie/all_equal_V{V}", np.full(V, 0.25, F32), Opt(top_k=10), cut=V // 2)
    # +0.0 and -0.0 mixed at the threshold
    lg = gauss(5, 64, 0.5, -2.0); lg[[3, 17, 40, 41, 60]] = F32(0.7)
    z = [1, 2, 8, 9, 20, 21, 22, 33, 34, 50, 51, 52, 61, 62, 63]
    lg[z] = np.where(np.arange(len(z)) % 2 == 0, F32(0.0), F32(-0.0))
    rr = build("tie/signed_zeros", lg, Opt(top_k=10), cut=12, targets=("first", "mid", "last", "edge"))
    assert all(x.n_keep == 20 and x.tie == 15 for x in rr)
    rows += rr
    # a tie set cut by top-p: the index order decides which of the equal entries survive
    lg = np.full(64, -9.0, F32); lg[[50, 7, 33]] = F32(2.0); lg[[60, 12, 45, 3, 28, 55, 19, 38, 9, 41]] = F32(1.0)
    rows += build("tie/cut_by_top_p", lg, Opt(), cut=6, targets=("first", "last", "edge"))
    return rows


def _key_rows():
    rows = []
    rows += build("key/all_negative", gauss(6, 300, 1.0, -20.0), Opt(top_k=50), cut=30)
    # neighbours one ulp apart at the threshold: the last radix pass separates them
    lg = gauss(7, 300); srt = np.argsort(-lg, kind="stable")
    lg[srt[50]] = np.nextafter(lg[srt[49]], NEG_INF)
    rr = build("key/ulp_neighbours", lg, Opt(top_k=50), targets=("first", "last", int(np.searchsorted(np.sort(srt[:50]), srt[49]))))
    assert all(x.n_keep == 50 for x in rr)
    rows += rr
    # values that differ only in the top byte (sign and the upper exponent bits): 4, 1, 0.25, -1, -4
    lg = np.tile(np.array([4.0, 1.0, 0.25, -1.0, -4.0], F32), 7)[:32]
    assert len({int(b) & 0x00ffffff for b in lg.view(np.uint32)}) == 1
    rr = build("key/top_byte_only", lg, Opt(top_k=12), cut=10)
    assert all(x.n_keep == 14 for x in rr)
    rows += rr
    # a subnormal pair at the threshold: 2 * 2^-149 is kept, 2^-149 is not
    lg = gauss(8, 64, 0.5, -3.0); lg[np.arange(9) * 7] = F32(0.5)
    sub = np.array([2, 1], np.uint32).view(F32); lg[30], lg[31] = sub[0], sub[1]
    rr = build("key/subnormal_pair", lg, Opt(top_k=10), targets=("first", "last", int(np.searchsorted(np.sort(np.r_[np.arange(9) * 7, 30]), 30))))
    assert all(x.n_keep == 10 for x in rr)
    rows += rr
    # top_k above the number of finite entries: the threshold is -inf, everything is kept, the rest at probability 0
    for V in (64, 1100):
        lg = np.full(V, NEG_INF, F32); f = np.sort(np.random.default_rng(9).permutation(V)[:20]); lg[f] = gauss(10, 20)
        rr = build(f"key/threshold_neg_inf_V{V}", lg, Opt(top_k=30), cut=15, targets=("first", "last", "edge"))
        assert all(x.n_keep == V for x in rr)
        rows += rr
    return rows


def _top_p_rows():
    rows = []
    lg = gauss(11, 300, 0.5)
    for k, cut in ((64, 64), (65, 64), (65, 65), (64, 63), (64, 1), (65, "n_keep")):
        rows += build(f"top_p/k{k}_cut{cut}", lg, Opt(top_k=k), cut=cut, targets=("first",) if cut == 1 else ("first", "mid", "last", "edge"))
    for tp in (1.0, 0.0):                                   # use_top_p off both ways
        rows += build(f"top_p/off_{tp}", lg, Opt(top_k=64, top_p=tp))
    # top_k 64 and 65 on the same row whose 65th entry has a probability far below the tolerance: same u, same id, the other sum path
    g = np.full(300, -60.0, F32) + gauss(12, 300, 0.1); top = np.sort(np.random.default_rng(13).permutation(300)[:64]); g[top] = gauss(14, 64, 0.5)
    a = build("top_p/k64_vs_k65/k64", g, Opt(top_k=64), cut=48, targets=("first", 5))
    rows += a
    for x in a:
        rows += fixed(x.name.replace("/k64/", "/k65/"), g, replace(x.opt, top_k=65), x.u, x.expect)
    # cum == top_p exactly: 4 equal logits, top_p = 0.5 -> the cut is 3 (first cum > top_p), not 2
    g = np.full(8, NEG_INF, F32); g[[1, 3, 4, 6]] = F32(0.5)
    rows += fixed("top_p/cum_equals_top_p", g, Opt(top_p=0.5), 0.9, 4, check_p=False)     # top_p decision exact: cum = 0.25, 0.5, 0.75, 1 under any expf
    return rows


def not_found_length():
    """smallest n >= 3 for which the float32 sequential sum of n x fl(1 / n) stays below 1"""
    for n in range(3, 200):
        if np.cumsum(np.full(n, F32(1.0) / F32(n), F32), dtype=F32)[-1] < F32(1.0):
            return n
    raise AssertionError("no such length")


def _u_rows():
    rows = []
    eq = "equal logits: e = 1 under any expf, the sum and its quotients are exact"
    g4 = np.full(16, NEG_INF, F32); g4[[2, 5, 11, 13]] = F32(1.25)
    g2 = np.full(16, NEG_INF, F32); g2[[6, 9]] = F32(-0.5)
    hot = np.full(2, NEG_INF, F32); hot[1] = F32(3.0)
    q = F32(0.25)
    rows += fixed("u/zero", gauss(15, 64), Opt(top_k=10), 0.0, 0, exact="u == 0 gives 0")
    rows += fixed("u/zero_index0_masked", g4, Opt(), 0.0, 0, exact="u == 0 gives 0, kept or not")
    rows += fixed("u/below_first_step", g4, Opt(), np.nextafter(q, F32(0)), 2, exact=eq)
    rows += fixed("u/on_first_step", g4, Opt(), q, 2, exact=eq)
    rows += fixed("u/above_first_step", g4, Opt(), np.nextafter(q, F32(1)), 5, exact=eq)
    rows += fixed("u/one_4_equal", g4, Opt(), 1.0, 13, exact=eq)
    rows += fixed("u/half_2_equal", g2, Opt(), 0.5, 6, exact=eq)
    rows += fixed("u/one_2_equal", g2, Opt(), 1.0, 9, exact=eq)
    rows += fixed("u/one_one_hot", hot, Opt(), 1.0, 1, exact="one finite logit: p = 1")
    n = not_found_length()
    g = np.full(n + 3, NEG_INF, F32); g[2:2 + n] = F32(0.75)
    rows += fixed(f"u/not_found_n{n}", g, Opt(), 1.0, 0, exact=eq + f"; the float32 running sum of {n} x fl(1/{n}) ends below 1")
    return rows


def _penalty_rows():
    rows = []
    V = 3072
    # seen entries at positive, negative and zero logits, sampled and greedy
    lg = gauss(16, V); lg[100] = F32(0.0); lg[200] = F32(2.5); lg[300] = F32(-1.5); lg[2150] = F32(1.0)
    sn = _seen(V, 100, 200, 300, 5, 6, 7)
    rows += build("pen/seen_signs", lg, Opt(temperature=0.9, top_k=50, rep=1.3, eos=2150), cut=30, seen=sn, tc=5, suppress=True,
                  targets=("first", "mid", "last", "edge"))
    g = np.full(V, -5.0, F32); g[40] = F32(2.0); g[41] = F32(1.9)
    for rep, want in ((1.3, 41), (1.0, 40), (1.0 + 1e-10, 40)):
        rows += fixed(f"pen/greedy_rep{rep}", g, Opt(temperature=0.0, rep=rep), 0.3, want, seen=_seen(V, 40), suppress=True, exact="greedy")
    g = np.full(V, -5.0, F32); g[40] = F32(-1.0); g[41] = F32(-1.2)        # negative logits are multiplied
    rows += fixed("pen/greedy_negative", g, Opt(temperature=0.0, rep=1.3), 0.3, 41, seen=_seen(V, 40), suppress=True, exact="greedy")
    # a zero logit is multiplied (0 * rep), not divided: with rep = 0 the quotient's factor is inf and 0 * inf is NaN
    g = np.full(64, -1.0, F32); g[9] = F32(0.0); g[20] = F32(-3.0)
    rows += fixed("pen/zero_logit_rep0_greedy", g, Opt(temperature=0.0, rep=0.0), 0.3, 9, seen=_seen(64, 9, 20), exact="greedy")
    rows += build("pen/zero_logit_rep0", g, Opt(top_k=5, rep=0.0), seen=_seen(64, 9, 20), targets=(9,))
    # EOS masking: eos inside / outside the suppressed range, none, different from codec_eos; tc = min_new - 1 and = min_new
    for eos, ce, name in ((2150, 2150, "inside"), (100, 2150, "outside"), (2200, 2150, "inside_not_codec_eos"), (None, 2150, "none")):
        g = np.full(V, -5.0, F32); g[50] = F32(1.0)
        if eos is not None:
            g[eos] = F32(3.0)
        for tc in (1, 2):
            unmasked = eos is not None and tc >= 2 and (eos < V - 1024 or eos == ce)
            rows += fixed(f"pen/eos_{name}_tc{tc}", g, Opt(temperature=0.0, eos=eos, min_new=2), 0.3, eos if unmasked else 50, tc=tc, codec_eos=ce,
                          suppress=True, exact="greedy")
    g = gauss(17, V); g[2150] = F32(4.0)
    for tc in (1, 2):
        rows += build(f"pen/eos_sampled_tc{tc}", g, Opt(temperature=0.9, top_k=50, eos=2150, min_new=2), cut=20, tc=tc, suppress=True)
    # the first suppressed index is V - 1024
    g = np.full(V, -5.0, F32); g[V - 1024] = F32(3.0); g[V - 1025] = F32(1.0)
    rows += fixed("pen/suppress_edge", g, Opt(temperature=0.0), 0.3, V - 1025, suppress=True, exact="greedy")
    # V < 1024: everything is suppressed except a codec_eos inside V
    g = gauss(18, 1000)
    rows += fixed("pen/small_vocab_greedy", g, Opt(temperature=0.0), 0.3, 700, codec_eos=700, suppress=True, exact="greedy")
    rows += fixed("pen/small_vocab_sampled", g, Opt(top_k=50, top_p=0.9), 0.6, 700, codec_eos=700, suppress=True, exact="one finite logit: p = 1")
    # greedy with ties, with and without penalties
    g = np.full(V, -2.0, F32); g[[5, 900]] = F32(1.5)
    rows += fixed("pen/greedy_tie", g, Opt(temperature=0.0, rep=1.3), 0.3, 5, suppress=True, exact="greedy")
    rows += fixed("pen/greedy_tie_penalised", g, Opt(temperature=0.0, rep=1.3), 0.3, 900, seen=_seen(V, 5), suppress=True, exact="greedy")
    return rows


_CONSTRUCTED = None


def constructed():
    """every constructed row, built once"""
    global _CONSTRUCTED
    if _CONSTRUCTED is None:
        _CONSTRUCTED = _size_rows() + _tie_rows() + _key_rows() + _top_p_rows() + _u_rows() + _penalty_rows()
        names = [r.name for r in _CONSTRUCTED]
        assert len(set(names)) == len(names)
    return _CONSTRUCTED


# ------------------------------------------------------------------------------------------------------------------ fuzz rows
# (V, top_k, top_p): 3.5 * N(0, 1) logits. A wide top-k with top-p on (4096 / 1500 / 0.99) measured 38 ambiguous rows of 256 — the
# cut lands among hundreds of entries of probability ~1e-6 — so that shape is reached by construction only (size/V4096/*).
FUZZ_CASES = ((3072, 0, 1.0), (3072, 50, 0.9), (2048, 65, 0.95))
FUZZ_ROWS, FUZZ_LAUNCH = 256, 64
_FUZZ = {}


def _allowed(row: Row):
    """every id the tolerance admits: cuts between cut(top_p -+ tol), and for each of them picks between pick(u -+ tol)"""
    h = host_row(row.opt)
    a = (row.logits, row.u, h, row.seen, row.tc, row.codec_eos, row.suppress)
    r32, r64 = sample_ref(*a, dt=F32), sample_ref(*a, dt=np.float64)
    cuts = {r64.cut}
    if h["use_top_p"]:
        t = tol_of(r32.cum, r64.cum)
        lo = int(np.searchsorted(r64.cum, float(h["top_p"]) - t, side="right")) + 1
        hi = int(np.searchsorted(r64.cum, float(h["top_p"]) + t, side="right")) + 1
        cuts = set(range(min(lo, r64.n_keep), min(hi, r64.n_keep) + 1))
    ids = set()
    for c in cuts:
        a32 = sample_ref(*a, dt=F32, force_cut=c); a64 = sample_ref(*a, dt=np.float64, force_cut=c)
        t = tol_of(a32.cdf, a64.cdf)
        u = float(F32(row.u))
        lo = int(np.searchsorted(a64.cdf, u - t, side="left")); hi = int(np.searchsorted(a64.cdf, u + t, side="left"))
        for k in range(lo, hi + 1):
            ids.add(int(a64.ids[k]) if k < a64.ids.size else 0)
    return r64, frozenset(ids)


def fuzz(case):
    """FUZZ_ROWS rows of one FUZZ_CASES entry, built once: random temperature, repetition penalty, seen mask, token count and u"""
    if case not in _FUZZ:
        V, k, p = case
        rng = np.random.default_rng(7919 * V + 31 * k + int(1000 * p))
        rows = []
        for i in range(FUZZ_ROWS):
            lg = (3.5 * rng.standard_normal(V)).astype(F32)
            opt = Opt(temperature=float(rng.choice([0.7, 0.9, 1.0, 1.3])), top_k=k, top_p=p, rep=float(rng.choice([1.0, 1.05, 1.3])), eos=2150, min_new=2)
            sn = (rng.random(V) < 0.05).astype(np.uint8)
            row = Row(f"fuzz/V{V}_k{k}_p{p}/{i}", lg, opt, float(F32(rng.random())), -1, sn, int(rng.integers(0, 4)), 2150, True)
            r64, ids = _allowed(row)
            row.expect, row.allowed = r64.id, ids
            assert row.expect in ids
            row.n_keep, row.cut, row.tie = r64.n_keep, r64.cut, r64.tie
            row.path = predict_path(r64.n_keep, r64.cut, r64.tie, k, V)
            rows.append(row)
        _FUZZ[case] = rows
    return _FUZZ[case]


def ambiguous(rows):
    return [r for r in rows if len(r.allowed) > 1]


# ------------------------------------------------------------------------------------------------------------------ launches
def launches(rows, per_launch=64):
    """rows grouped into launches: one vocabulary, one suppression setting and one codec_eos per launch (launch-wide arguments)"""
    groups = {}
    for r in rows:
        groups.setdefault((r.V, r.suppress, r.codec_eos), []).append(r)
    out = []
    for key in sorted(groups, key=lambda k: (k[0], k[1], k[2])):
        g = groups[key]
        out += [g[i:i + per_launch] for i in range(0, len(g), per_launch)]
    return out


# ------------------------------------------------------------------------------------------------------------------ session form
@dataclass
class SessionCase:
    """one launch in the form a session gives it: padded logits, strided draws, per-row records, counters, limits, held rows, history"""
    rows: list                       # Row per sequence (its own options)
    state: list                      # per sequence: "live" | "frozen" | "held" | "held_frozen"
    V: int
    ld: int
    max_frames: int
    u_stride: int
    hist_cap: int
    hist_stride_b: int
    frame_idx: np.ndarray
    pos: np.ndarray
    token_count: np.ndarray
    limit: np.ndarray
    text_ready: np.ndarray
    scalar: Opt = field(default_factory=Opt)


def session_case():
    V, MF = 1100, 9
    base = gauss(19, V, 0.7); base[0] = F32(-30.0)                 # id 0 is never a target: a wrong draw (poison, not found) shows
    opts = [Opt(temperature=0.9, top_k=50, top_p=0.9, rep=1.05, eos=1050, min_new=2),
            Opt(temperature=0.0, top_k=50, top_p=0.9, rep=1.3),                               # greedy
            Opt(temperature=1.0, top_k=0, top_p=0.9),                                         # no top-k
            Opt(temperature=1.3, top_k=64, top_p=1.0, rep=1.3),
            Opt(temperature=0.7, top_k=65, top_p=0.95, eos=3, min_new=4),
            Opt(temperature=0.9, top_k=2, top_p=0.5),
            Opt(temperature=1.0, top_k=1099, top_p=0.8, rep=1.05),
            Opt(temperature=0.9, top_k=50, top_p=0.0, eos=1050, min_new=1)]
    states = ["live"] * 8 + ["frozen", "held", "held_frozen", "live"]
    opts += [opts[0], opts[3], opts[4], opts[0]]
    tcs = [0, 1, 2, 3, 4, 5, 1, 2, 4, 2, 3, 7]                      # row 11: token_count >= hist_cap, its history slot is left alone
    rows = []
    for b, (o, tc) in enumerate(zip(opts, tcs)):
        lg = np.roll(base[1:], 37 * b); lg = np.r_[base[:1], lg].astype(F32)
        lg[1050] = F32(2.5)                                          # the EOS id of rows 0 and 7 is a likely pick unless masked
        sn = (np.random.default_rng(100 + b).random(V) < 0.1).astype(np.uint8)
        if host_row(o)["greedy"]:
            v = values(lg, host_row(o), sn, tc, 1050, True)
            rows += fixed(f"session/{b}", lg, o, 0.5, _first_max(v), seen=sn, tc=tc, codec_eos=1050, suppress=True, exact="greedy")
        else:
            cut = None if not host_row(o)["use_top_p"] else 1 if o.top_k == 2 else 12
            r = build(f"session/{b}", lg, o, cut=cut, seen=sn, tc=tc, codec_eos=1050, suppress=True, targets=("first",) if cut == 1 else ("mid",))
            rows += r
    assert all(r.expect != 0 for r in rows)
    fi = np.array([0, 1, 2, 3, 4, 5, 6, 7, 4, 3, 5, 8], np.int32)
    lim = np.array([9, 9, 9, 9, 9, 9, 9, 8, 4, 9, 5, 9], np.int32)
    rdy = np.array([2 ** 31 - 1] * 8 + [2 ** 31 - 1, 3, 5, 2 ** 31 - 1], np.int32)
    for b, st in enumerate(states):
        assert (fi[b] >= lim[b]) == ("frozen" in st) and (fi[b] >= rdy[b]) == ("held" in st)
    return SessionCase(rows, states, V, V + 12, MF, MF + 2, 6, 6 * V + 5, fi, (fi + 40 + np.arange(12)).astype(np.int32),
                       np.array(tcs, np.int32), lim, rdy, Opt(temperature=0.0, top_k=3, top_p=0.2, rep=2.0, eos=7, min_new=9))
