"""Op-level tests of k_sample in the forms a session launches it (-m gpu): ONE launch_sample per call through q3_sample_ex, ids against
the numpy restatement of the sampler in sampler_cases.py. What needs no GPU — the reference on hand-worked rows, the margin of every
constructed row, the path coverage of the table, the ambiguity cap, the mutants the table detects — is in test_sampler_reference.py.

Constructed rows (top_p and u placed at midpoints, at least 4 x the float32 / float64 deviation of that row from any step): the id must
be equal. Fuzz rows (random u): equal, or inside the row's tolerance set, and at most 5 % of a case may be ambiguous. Every buffer the
kernel may write goes in with guard elements around it: guards must come back intact, `seen` changes in exactly the sampled byte, the
counters of every row are checked. The session form adds padded logits with NaN in the padding, strided draws with poison in every
other slot, eight different per-row records under scalar fields that say the opposite, frozen and held rows, and the logits history.

Measured on an MI355X: 388 constructed rows and the 12 of the session form, all equal; 768 fuzz rows, 3 ambiguous by the CPU analysis
(all three gave the float64 reference's id). No row missed a check."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import sampler_cases as S
from sampler_cases import F32

pytestmark = pytest.mark.gpu

G = 8
COUNTS = {"constructed": 0, "fuzz": 0, "ambiguous": 0, "ambiguous and another id than float64": 0}
TOK_SENTINEL = np.uint32(0xFFFFFFF0)
HIST_BITS = np.uint32(0x7FC0BEEF)


@pytest.fixture(scope="module", autouse=True)
def _counts():
    yield
    print(f"\nk_sample rows checked: {COUNTS}")


def _opts(o):
    return q.SynthesisOptions(temperature=o.temperature, top_k=o.top_k, top_p=o.top_p, repetition_penalty=o.rep, eos_token_id=o.eos, min_new_tokens=o.min_new)


def _rec(o):
    return q.sample_row(_opts(o))


def _guarded(body, sentinel, dtype):
    return np.r_[np.full(G, sentinel, dtype), np.asarray(body, dtype).reshape(-1), np.full(G, sentinel, dtype)]


def run_rows(rows, scalar=False):
    """one launch over rows of one vocabulary; per-row records and device token counts, or (scalar) one row through the scalar fields and
    the static token count. Returns the ids after the state checks every launch gets."""
    B, V = len(rows), rows[0].V
    assert len({(r.V, r.suppress, r.codec_eos) for r in rows}) == 1 and (not scalar or B == 1)
    lg = np.stack([r.logits for r in rows])
    u = np.array([r.u for r in rows], F32)
    seen0 = np.stack([r.seen if r.seen is not None else np.zeros(V, np.uint8) for r in rows])
    tok = _guarded(np.full(B, TOK_SENTINEL), TOK_SENTINEL, np.uint32)
    seen = _guarded(seen0, 0xA5, np.uint8)
    tc0 = np.array([r.tc for r in rows], np.int32)
    tc = _guarded(tc0, -77, np.int32)
    if scalar:
        kw = dict(scalar=_rec(rows[0].opt), token_count_static=int(tc0[0]))
    else:               # the scalar fields say greedy: a launch that ignored its records would show at once
        kw = dict(scalar=_rec(S.Opt(temperature=0.0)), rows=[_rec(r.opt) for r in rows], token_count=tc)
    q.sample_ex(lg, u, V, tok, seen=seen, codec_eos=rows[0].codec_eos, use_suppress=rows[0].suppress, guard=G, **kw)
    ids = tok[G:-G].astype(np.int64)
    assert (tok[:G] == TOK_SENTINEL).all() and (tok[-G:] == TOK_SENTINEL).all() and (ids < V).all(), "tok guards / range"
    assert (seen[:G] == 0xA5).all() and (seen[-G:] == 0xA5).all(), "seen guards"
    after = seen[G:-G].reshape(B, V)
    for b in range(B):
        want = seen0[b].copy(); want[ids[b]] = 1
        assert (after[b] == want).all(), f"{rows[b].name}: seen changed at {np.flatnonzero(after[b] != seen0[b])}, sampled {ids[b]}"
    assert (tc[:G] == -77).all() and (tc[-G:] == -77).all() and (scalar or (tc[G:-G] == tc0 + 1).all()), "token counts"
    return ids


@pytest.fixture(scope="module")
def constructed_ids():
    """every constructed row's id, one launch per group of the table, run once and shared"""
    out = {}
    for launch in S.launches(S.constructed()):
        for r, i in zip(launch, run_rows(launch)):
            out[r.name] = int(i)
    return out


def test_constructed_rows_give_the_expected_id(constructed_ids):
    rows = S.constructed()
    COUNTS["constructed"] += len(rows)
    wrong = [(r.name, constructed_ids[r.name], r.expect, r.path) for r in rows if constructed_ids[r.name] != r.expect]
    assert not wrong, f"{len(wrong)} of {len(rows)} rows: {wrong[:12]}"


def test_boundaries_on_identical_rows(constructed_ids):
    """both sides of a two-sided boundary on rows that differ in nothing else give the same id"""
    for a, b in (("top_p/k64_vs_k65/k64/first", "top_p/k64_vs_k65/k65/first"), ("top_p/k64_vs_k65/k64/5", "top_p/k64_vs_k65/k65/5"),
                 ("tie/nsel1024/first", "tie/nsel1025/first"), ("tie/nsel1024/mid", "tie/nsel1025/mid"), ("tie/nsel1024/1000", "tie/nsel1025/1000")):
        assert constructed_ids[a] == constructed_ids[b], (a, b, constructed_ids[a], constructed_ids[b])


def test_scalar_fields_and_static_token_count(constructed_ids):
    """rows = NULL, token_count = NULL: the same row alone through the scalar fields gives the id of the per-row launch"""
    rows = S.constructed()[::11]
    assert len(rows) >= 30
    for r in rows:
        assert int(run_rows([r], scalar=True)[0]) == constructed_ids[r.name] == r.expect, r.name


@pytest.mark.parametrize("case", S.FUZZ_CASES, ids=lambda c: f"V{c[0]}_k{c[1]}_p{c[2]}")
def test_fuzz_rows(case):
    rows = S.fuzz(case)
    amb = len(S.ambiguous(rows))
    assert amb <= S.FUZZ_CAP * len(rows)
    other = 0
    ids37 = None
    for k in range(0, len(rows), S.FUZZ_LAUNCH):
        launch = rows[k:k + S.FUZZ_LAUNCH]
        ids = run_rows(launch)
        for r, i in zip(launch, ids):
            assert int(i) in r.allowed or int(i) == r.expect, f"{r.name}: id {i}, expected {r.expect}, tolerance set {sorted(r.allowed)}"
            other += int(i) != r.expect
        if k == 0:
            ids37 = (launch[37], int(ids[37]))
    # a row alone and the same row as row 37 of a 64-row launch
    assert int(run_rows([ids37[0]])[0]) == ids37[1]
    COUNTS["fuzz"] += len(rows); COUNTS["ambiguous"] += amb; COUNTS["ambiguous and another id than float64"] += other
    print(f"{case}: {len(rows)} rows, {amb} ambiguous, {other} with a neighbour's id")


def test_plain_sample_entry_is_unchanged():
    """token_count < 0 through q3_sample: no penalty pipeline — the mask, the repetition penalty, EOS and suppression are ignored"""
    lg = S.gauss(77, 3072)
    rows = S.build("plain", lg, S.Opt(temperature=0.9, top_k=50), cut=30)
    o = _opts(S.replace(rows[0].opt, rep=1.3, eos=rows[0].expect, min_new=5))
    ids = q.sample(np.stack([r.logits for r in rows]), np.array([r.u for r in rows], F32), o, seen=np.ones((len(rows), 3072), np.uint8), token_count=-1)
    assert [int(i) for i in ids] == [r.expect for r in rows]
    assert any(r.expect >= 2048 for r in rows)              # suppression would have shown


def test_session_form():
    c = S.session_case()
    B, V = len(c.rows), c.V
    lg = np.full((B, c.ld), np.nan, F32); lg[:, :V] = np.stack([r.logits for r in c.rows])
    u = np.full(B * c.u_stride, np.nan, F32)
    u[np.arange(B) * c.u_stride + c.token_count] = [r.u for r in c.rows]
    seen0 = np.stack([r.seen for r in c.rows])
    tok0 = (4000 + np.arange(B)).astype(np.uint32)
    tok, seen = _guarded(tok0, TOK_SENTINEL, np.uint32), _guarded(seen0, 0xA5, np.uint8)
    tc, fi, pos = _guarded(c.token_count, -77, np.int32), _guarded(c.frame_idx, -78, np.int32), _guarded(c.pos, -79, np.int32)
    hist = _guarded(np.full(B * c.hist_stride_b, HIST_BITS, np.uint32), HIST_BITS, np.uint32).view(F32)
    q.sample_ex(lg, u, V, tok, _rec(c.scalar), rows=[_rec(r.opt) for r in c.rows], seen=seen, u_stride=c.u_stride, draw_idx=c.token_count,
                token_count=tc, advance=True, frame_idx=fi, pos=pos, limit=c.limit, text_ready=c.text_ready, logits_hist=hist,
                hist_stride_b=c.hist_stride_b, hist_cap=c.hist_cap, codec_eos=1050, use_suppress=True, guard=G)
    for name, buf, s in (("tok", tok, TOK_SENTINEL), ("seen", seen, 0xA5), ("token_count", tc, -77), ("frame_idx", fi, -78), ("pos", pos, -79)):
        assert (buf[:G] == s).all() and (buf[-G:] == s).all(), f"{name} guards"
    after = seen[G:-G].reshape(B, V)
    for b, (r, st) in enumerate(zip(c.rows, c.state)):
        got = (int(tok[G + b]), int(tc[G + b]), int(fi[G + b]), int(pos[G + b]))
        if "held" in st:               # held (also when frozen as well): token, mask and counters bit-identical to the input
            assert got == (int(tok0[b]), c.token_count[b], c.frame_idx[b], c.pos[b]) and (after[b] == seen0[b]).all(), (b, st, got)
            continue
        step = 0 if st == "frozen" else 1          # frozen: counters stay, tok and seen are still written
        assert got == (r.expect, c.token_count[b] + step, c.frame_idx[b] + step, c.pos[b] + step), (b, st, got, r.expect)
        assert seen0[b, r.expect] == 0 and list(np.flatnonzero(after[b] != seen0[b])) == [r.expect], (b, st)
    hb = hist.view(np.uint32)
    want = np.full(hb.shape, HIST_BITS, np.uint32)
    for b in range(B):
        t = int(c.token_count[b])
        if t < c.hist_cap:
            at = G + b * c.hist_stride_b + t * V
            want[at:at + V] = c.rows[b].logits.view(np.uint32)
    assert (hb == want).all(), f"logits_hist differs at {np.flatnonzero(hb != want)[:8]}"
    COUNTS["constructed"] += B
