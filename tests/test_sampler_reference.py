"""What the op-level sampler tests rest on, checked without a GPU (sampler_cases.py): the reference against hand-worked rows, the
construction rule (every constructed row keeps its margin), the case table against the kernel's paths (every combination that can occur
is reached), the ambiguity cap of the committed fuzz seeds, and the table's power: each deliberate change of the reference ("mutant")
alters the expected id of at least one constructed row. The entry's refusals come back as Q3_INVALID_ARG before any device call."""
import collections

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
import sampler_cases as S
from sampler_cases import F32, Opt


def test_reference_on_hand_worked_rows():
    # logits ln 4, ln 2, ln 1, ln 1 -> p = 1/2, 1/4, 1/8, 1/8 (exact powers of two up to exp's rounding; the steps are far from u)
    lg = np.log(np.array([1.0, 4.0, 1.0, 2.0])).astype(F32)
    h = S.host_row(Opt())
    assert [S.sample_ref(lg, u, h, suppress=False).id for u in (0.1, 0.2, 0.6, 0.7, 0.8, 0.9)] == [0, 1, 1, 2, 3, 3]
    # top-k 2 keeps ids 1 and 3 (p = 2/3, 1/3); top-p 0.6 then cuts to id 1 alone (cum 2/3 > 0.6 at the first entry)
    h = S.host_row(Opt(top_k=2))
    r = S.sample_ref(lg, 0.7, h, suppress=False)
    assert (r.id, r.n_keep, r.cut, list(r.order)) == (3, 2, 2, [1, 3])
    r = S.sample_ref(lg, 0.7, S.host_row(Opt(top_k=2, top_p=0.6)), suppress=False)
    assert (r.id, r.cut) == (1, 1)
    # ties at the threshold all survive; top-p over the sorted row orders equal values by index
    r = S.sample_ref(lg, 0.99, S.host_row(Opt(top_k=3)), suppress=False)
    assert (r.n_keep, r.tie, list(r.order), r.id) == (4, 2, [1, 3, 0, 2], 3)
    # penalty: positive divided, negative and zero multiplied; then the first maximum
    g = np.array([2.0, -1.0, 0.0, 1.6], F32)
    v = S.values(g, S.host_row(Opt(rep=1.25)), np.array([1, 1, 1, 0], np.uint8), suppress=False)
    assert list(v) == [F32(2.0) * (F32(1) / F32(1.25)), F32(-1.25), F32(0.0), F32(1.6)] and S._first_max(v) == 0
    # u == 0 and "not found" give 0
    assert S.sample_ref(lg, 0.0, S.host_row(Opt()), suppress=False).id == 0
    assert S.sample_ref(np.full(4, -np.inf, F32), 0.5, S.host_row(Opt(temperature=0.0)), suppress=False).id == 0


def test_host_row_is_the_sessions_record():
    """the cases' restatement of sample_row() against the library's own (q3_sample_row, host only)"""
    opts = {r.opt for r in S.constructed()} | {r.opt for r in S.session_case().rows} | {S.session_case().scalar}
    assert len(opts) > 60
    for o in opts:
        rec = q.sample_row(q.SynthesisOptions(temperature=o.temperature, top_k=o.top_k, top_p=o.top_p, repetition_penalty=o.rep,
                                              eos_token_id=o.eos, min_new_tokens=o.min_new))
        h = S.host_row(o)
        for name, val in h.items():
            got = getattr(rec, name)
            same = np.array(got, F32).view(np.uint32) == np.array(val, F32).view(np.uint32) if isinstance(val, F32) else got == val
            assert same, (o, name, got, val)
        assert rec.pad == 0


def test_case_table_reaches_every_path():
    rows = S.constructed()
    with_top_p = {r.path for r in rows if S.host_row(r.opt)["use_top_p"]}
    assert with_top_p >= S.ALL_PATHS, S.ALL_PATHS - with_top_p
    assert {r.path for r in rows} >= S.ALL_PATHS | {("greedy",)}
    # the sizes and widths the table promises
    sizes = collections.defaultdict(set)
    for r in rows:
        if r.name.startswith("size/"):
            sizes[r.V].add(r.opt.top_k)
    assert set(sizes) == set(S.SIZES_V)
    for V, ks in sizes.items():
        assert ks == {0, 1, 2, 50, 63, 64, 65, V - 1, V, V + 5}, V
    # both sides of every two-sided boundary
    by = {r.name: r for r in rows}
    assert by["tie/nsel1024/first"].path[0] == "radix" and by["tie/nsel1025/first"].path[0] == "bitonic"
    assert (by["tie/nsel1024/first"].n_keep, by["tie/nsel1025/first"].n_keep) == (1024, 1025)
    assert by["top_p/k64_cut64/first"].path == ("radix", "wave", "wave") and by["top_p/k65_cut64/first"].path == ("radix", "thread", "wave")
    assert by["top_p/k65_cut65/first"].path == ("radix", "thread", "thread")
    assert by["top_p/k64_vs_k65/k64/first"].expect == by["top_p/k64_vs_k65/k65/first"].expect
    assert by["top_p/k64_vs_k65/k64/first"].path[1] == "wave" and by["top_p/k64_vs_k65/k65/first"].path[1] == "thread"
    assert by["key/threshold_neg_inf_V64/first"].n_keep == 64 and by["key/threshold_neg_inf_V1100/first"].path[0] == "bitonic"
    assert by["top_p/k64_cut1/first"].cut == 1 and by["top_p/k65_cutn_keep/first"].cut == 65
    assert not S.host_row(by["top_p/off_1.0/first"].opt)["use_top_p"] and not S.host_row(by["top_p/off_0.0/first"].opt)["use_top_p"]


def test_every_constructed_row_keeps_its_margin():
    rows = S.constructed()
    assert len(rows) > 300
    worst = min(r.margin for r in rows if not r.exact)
    print(f"constructed rows: {len(rows)}, smallest margin {worst:.1f} x tolerance")
    for r in rows:
        assert r.exact or r.margin >= 1.0, (r.name, r.margin)
        assert r.ref(F32).id == r.expect and (r.exact or r.ref(np.float64).id == r.expect), r.name
        assert r.logits.size <= 4096
    for launch in S.launches(rows):
        assert len(launch) <= 64 and len({(r.V, r.suppress, r.codec_eos) for r in launch}) == 1


def test_not_found_row():
    n = S.not_found_length()
    c = np.cumsum(np.full(n, F32(1.0) / F32(n), F32), dtype=F32)
    assert c[-1] < F32(1.0) and n >= 3
    row = [r for r in S.constructed() if r.name.startswith("u/not_found")][0]
    assert row.expect == 0 and row.logits[0] == -np.inf and row.ref(F32).cdf[-1] < 1.0


@pytest.mark.parametrize("case", S.FUZZ_CASES, ids=lambda c: f"V{c[0]}_k{c[1]}_p{c[2]}")
def test_fuzz_ambiguity_stays_under_the_cap(case):
    rows = S.fuzz(case)
    amb = S.ambiguous(rows)
    print(f"{case}: {len(amb)} ambiguous rows of {len(rows)}")
    assert len(rows) == S.FUZZ_ROWS and len(amb) <= S.FUZZ_CAP * len(rows)
    for r in rows:
        assert r.expect in r.allowed, (r.name, r.allowed)
        assert r.ref(np.float64).id == r.expect
        assert len(r.allowed) > 1 or r.ref(F32).id == r.expect, r.name


@pytest.mark.parametrize("mutant", S.MUTANTS)
def test_the_table_detects_a_wrong_sampler(mutant):
    """the float32 reference with one deliberate change must give another id on at least one constructed row"""
    caught = [r.name for r in S.constructed() if r.ref(F32, mutant).id != r.expect]
    print(f"{mutant}: {len(caught)} rows differ, e.g. {caught[:4]}")
    assert caught, mutant


def test_session_case_is_what_it_says():
    c = S.session_case()
    B = len(c.rows)
    assert B == 12 and len({r.opt for r in c.rows[:8]}) == 8 and c.ld == c.V + 12 and c.u_stride == c.max_frames + 2
    h = [S.host_row(r.opt) for r in c.rows[:8]]
    assert sum(x["greedy"] for x in h) == 1 and sum(x["top_k"] == 0 for x in h) == 1
    s = S.host_row(c.scalar)
    assert s["greedy"] and s["top_k"] > 0                                     # the scalar fields say the opposite of rows 1 and 2
    assert collections.Counter(c.state) == {"live": 9, "frozen": 1, "held": 1, "held_frozen": 1}
    assert (c.token_count < c.u_stride).all() and (c.token_count >= c.hist_cap).sum() == 1 and c.hist_stride_b >= c.hist_cap * c.V
    assert all(r.expect != 0 and r.V == c.V and r.suppress and r.codec_eos == 1050 for r in c.rows)


def test_sample_ex_refuses_bad_arguments_before_any_device_call():
    assert _lib.ctypes.sizeof(_lib.CSampleRow) == 12 * 4 and _lib.ctypes.sizeof(_lib.CSampleEx) == 12 * 4 + 48 + 12 * 8
    rec = q.sample_row(q.SynthesisOptions())
    z = lambda n, dt=np.float32: np.zeros(n, dt)
    tok = z(2, np.uint32)
    bad = [lambda: q.sample_ex(z((2, 1)), z(2), 1, tok, rec),                                                  # vocab < 2
           lambda: q.sample_ex(z((2, 4097)), z(2), 4097, tok, rec),                                            # vocab > 4096
           lambda: q.sample_ex(z((2, 8)), z(2), 9, tok, rec),                                                  # ld < vocab
           lambda: q.sample_ex(z((2, 8)), z(2), 8, tok, rec, u_stride=2),                                      # row 1 draws u[2] of 2
           lambda: q.sample_ex(z((2, 8)), z(4), 8, tok, rec, u_stride=2, draw_idx=[0, 2]),                     # u[4] of 4
           lambda: q.sample_ex(z((2, 8)), z(4), 8, tok, rec, u_stride=2, draw_idx=[-1, 0]),
           lambda: q.sample_ex(z((2, 8)), z(2), 8, tok, rec, advance=True),                                    # no counters
           lambda: q.sample_ex(z((2, 8)), z(2), 8, tok, rec, logits_hist=z(2 * 15), hist_stride_b=15, hist_cap=2),       # stride < cap * vocab
           lambda: q.sample_ex(z((2, 8)), z(2), 8, tok, rec, logits_hist=z(2 * 16), hist_stride_b=16, hist_cap=2, token_count_static=-1)]
    for k, call in enumerate(bad):
        with pytest.raises(_lib.Q3Error) as e:
            call()
        assert e.value.status == 1, k
    assert _lib.lib.q3_sample_ex(0, None) == 1 and _lib.lib.q3_sample_row(None, None) == 1
    a = _lib.CSampleEx()
    assert _lib.lib.q3_sample_ex(0, _lib.ctypes.byref(a)) == 1
    if _lib.lib.q3_device_count() <= 0:                    # a good call reaches the device and fails there: no CPU path
        with pytest.raises(_lib.Q3Error) as e:
            q.sample_ex(z((2, 8)), z(2), 8, tok, rec)
        assert e.value.status == 5
