"""q3_session_next_chunks: next_chunk_row for every row in one call, the rows' vocoder passes batched through the
session's codec stream. Chunks, boundaries and `done` flags are those of the per-row calls, and in continuous stream mode the
chunks of a row concatenate to its whole-utterance decode — the same BITS (np.array_equal on float32 PCM, no tolerance).
Tiny LM; the production decoder (bf16x3 kernels) and q.tiny()'s (the fallback kernels)."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt

SPF = 1920


def _full_decoder_cfg():
    t = q.tiny()
    return q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads,
                      n_kv_heads=t.n_kv_heads, cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers,
                      cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads, name="tiny-lm-full-decoder")


@pytest.fixture(scope="module", params=["production", "tiny"])
def gm(request):
    m = q.Qwen3TTS.from_synthetic(_full_decoder_cfg() if request.param == "production" else q.tiny(), seed=1234)
    yield m
    m.close()


def _session(gm, utts, opts, mode):
    s = gm.session(utts, opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, mode))
    return s


def _rounds(s, batched, rows=None, max_rounds=64):
    """chunk rounds until every row reports done: [[(samples or None, done) per row] per round]"""
    out = []
    for _ in range(max_rounds):
        r = s.next_chunks() if batched else [s.next_chunk_row(b) for b in range(s.B)]
        out.append([(None if a is None else a.samples, d) for a, d in r])
        if all(d for _, d in out[-1]):
            return out
    raise AssertionError("the session did not finish")


def _same_rounds(got, want):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        for b, ((ga, gd), (wa, wd)) in enumerate(zip(g, w)):
            assert gd == wd, (k, b)
            assert (ga is None) == (wa is None), (k, b)
            if ga is not None:
                np.testing.assert_array_equal(ga, wa, err_msg=f"round {k} row {b}")


def _cat(rounds, b):
    parts = [r[b][0] for r in rounds if r[b][0] is not None]
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def _utts(limits, base=0):
    return [q.Utterance(synthetic_prompt(8 + 3 * i, base + i), q.Speaker.Ryan, q.Language.English, seed=100 + base + i, max_length=L)
            for i, L in enumerate(limits)]


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_same_chunks_as_next_chunk_row(gm, mode):
    """Three rows with limits 23 / 10 / 17, chunk 7: every row gets the chunks, boundaries and done flags next_chunk_row gives on
    a twin session; in stream mode 1 the concatenation is the whole decode."""
    limits = [23, 10, 17]
    opts = q.SynthesisOptions(max_length=23, seed=42, eos_token_id=None, chunk_frames=7)
    s = _session(gm, _utts(limits), opts, mode); t = _session(gm, _utts(limits), opts, mode)
    got = _rounds(s, True); want = _rounds(t, False)
    _same_rounds(got, want)
    for b, L in enumerate(limits):
        sizes = [len(r[b][0]) // SPF for r in got if r[b][0] is not None]
        assert sizes == [7] * (L // 7) + ([L % 7] if L % 7 else []), (b, sizes)
        if mode == 1:
            np.testing.assert_array_equal(_cat(got, b), s.decode(b), err_msg=f"row {b}")
    s.close(); t.close()


@pytest.mark.gpu
@pytest.mark.parametrize("rows,frames,chunk", [(5, 75, 10), (17, 24, 12)])
def test_rows_equal_whole_decode(gm, rows, frames, chunk):
    """Five rows x 75 frames (on the production decoder the longest case of the suite) and a wide session of 17 rows."""
    opts = q.SynthesisOptions(max_length=frames, seed=7, eos_token_id=None, chunk_frames=chunk)
    s = _session(gm, _utts([frames] * rows, base=20), opts, 1)
    got = _rounds(s, True)
    for b in range(rows):
        a = _cat(got, b)
        assert a.shape == (frames * SPF,)
        np.testing.assert_array_equal(a, s.decode(b), err_msg=f"row {b}")
    s.close()


def _single(gm, utt, opts):
    """the row's own batch-1 streaming session, continuous mode: its chunks"""
    s = _session(gm, [utt], opts, 1)
    out = []
    for _ in range(64):
        a, d = s.next_chunk_row(0)
        if a is not None:
            out.append(a.samples)
        if d:
            s.close()
            return out
    raise AssertionError("the session did not finish")


@pytest.mark.gpu
def test_rows_that_leave_the_plain_path(gm):
    """One session, chunk 10: row 1 ends at 20 and is replaced when the others are at frame 30 (its state starts over at frame 0
    beside them); row 2 is an ICL row (context-free chunks, as next_chunk_row gives it); row 3 has a live EOS id and ends
    inside a chunk. Every row is held to its own batch-1 streaming session."""
    cfg = gm.config
    rng = np.random.default_rng(8)
    ref = rng.integers(0, 2048, size=(5, 16)).astype(np.uint32); ref[:, 0] = rng.integers(0, 3072, 5)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)
    opts = q.SynthesisOptions(max_length=60, seed=3, eos_token_id=None, chunk_frames=10)
    plain = q.Utterance(synthetic_prompt(9, 1), q.Speaker.Ryan, q.Language.English, seed=11, max_length=60)
    short = q.Utterance(synthetic_prompt(7, 2), q.Speaker.Ryan, q.Language.English, seed=12, max_length=20)
    later = q.Utterance(synthetic_prompt(11, 3), q.Speaker.Ryan, q.Language.English, seed=13, max_length=25)
    icl = q.Utterance(synthetic_prompt(6, 4), language=q.Language.French, xvector=xv, ref_codes=ref, ref_text_ids=synthetic_prompt(3, 5),
                      seed=14, max_length=30)
    # an EOS id that ends the row inside a chunk: the first semantic code of a frame 13 .. 38 (not a multiple of 10) that no
    # earlier frame of the free run has
    free = q.Utterance(synthetic_prompt(10, 6), q.Speaker.Ryan, q.Language.English, seed=15, max_length=40)
    s1 = gm.session([free], opts); s1.prefill(); s1.generate(40); c0 = s1.codes(0)[:, 0]; s1.close()
    f = next(f for f in range(13, 39) if f % 10 and c0[f] not in c0[:f])
    eos_opts = q.SynthesisOptions(max_length=40, seed=15, eos_token_id=int(c0[f]), chunk_frames=10)
    eos = q.Utterance(synthetic_prompt(10, 6), q.Speaker.Ryan, q.Language.English, seed=15, max_length=40, options=eos_opts)

    want = {"plain": _single(gm, plain, opts), "short": _single(gm, short, opts), "later": _single(gm, later, opts),
            "icl": _single(gm, icl, opts), "eos": _single(gm, eos, opts)}
    n_eos = sum(len(c) for c in want["eos"]) // SPF
    assert 0 < n_eos < 40 and n_eos % 10, n_eos                    # ... it did end inside a chunk

    s = _session(gm, [plain, short, icl, eos], opts, 1)
    got = {"plain": [], "short": [], "later": [], "icl": [], "eos": []}
    names = ["plain", "short", "icl", "eos"]
    for k in range(64):
        if k == 3:
            assert s.frames(0)[0] >= 30 and s.frames(1)[1]
            s.replace(1, later); names[1] = "later"
        r = s.next_chunks()
        for b, (a, d) in enumerate(r):
            if a is not None:
                got[names[b]].append(a.samples)
        if k >= 3 and all(d for _, d in r):
            break
    s.close()
    for nme in got:
        assert [len(c) for c in got[nme]] == [len(c) for c in want[nme]], nme
        np.testing.assert_array_equal(np.concatenate(got[nme]), np.concatenate(want[nme]), err_msg=nme)


@pytest.mark.gpu
def test_held_open_text_row(gm):
    """A row whose text is open and does not reach a whole chunk returns (None, False) while the other advances; after its
    appends its audio is the closed run's."""
    L = 21
    utts = [q.Utterance(synthetic_prompt(10, 7 + i), q.Speaker.Ryan, q.Language.English, seed=7 + i) for i in range(2)]
    opts = q.SynthesisOptions(max_length=L, seed=42, eos_token_id=None, chunk_frames=7)
    c = _session(gm, utts, opts, 1); c.prefill(); c.generate(L)
    ref = [c.decode(b) for b in range(2)]; c.close()
    first = api.Utterance(**{f: getattr(utts[1], f) for f in utts[1].__dataclass_fields__})
    first.text_ids = list(utts[1].text_ids)[:1]
    s = _session(gm, [utts[0], first], opts, 1)
    s.open_text(1); s.prefill()
    got = [[], []]
    r = s.next_chunks()
    assert r[0][0] is not None and len(r[0][0]) == 7 * SPF and not r[0][1]
    assert r[1] == (None, False)
    got[0].append(r[0][0].samples)
    s.append_text(1, list(utts[1].text_ids)[1:4])                 # three more frames: still less than a chunk
    r = s.next_chunks()
    assert r[1] == (None, False) and r[0][0] is not None
    got[0].append(r[0][0].samples)
    s.append_text(1, list(utts[1].text_ids)[4:], last=True)
    for _ in range(16):
        r = s.next_chunks()
        for b in range(2):
            if r[b][0] is not None:
                got[b].append(r[b][0].samples)
        if all(d for _, d in r):
            break
    s.close()
    for b in range(2):
        np.testing.assert_array_equal(np.concatenate(got[b]), ref[b], err_msg=f"row {b}")


@pytest.mark.gpu
def test_alternating_with_next_chunk_row(gm):
    """next_chunk_row(b) for some rows between next_chunks() calls: the rows' states fall behind their positions and catch up."""
    L = 45
    opts = q.SynthesisOptions(max_length=L, seed=5, eos_token_id=None, chunk_frames=7)
    s = _session(gm, _utts([L] * 3, base=40), opts, 1)
    got = [[], [], []]
    done = [False] * 3
    for k in range(32):
        if k % 2 == 0:
            r = s.next_chunks()
        else:
            r = [s.next_chunk_row(b) if b != 1 else (None, done[1]) for b in range(3)]      # rows 0 and 2 only
        for b, (a, d) in enumerate(r):
            if a is not None:
                got[b].append(a.samples)
            done[b] = d
        if all(done):
            break
    assert all(done)
    for b in range(3):
        np.testing.assert_array_equal(np.concatenate(got[b]), s.decode(b), err_msg=f"row {b}")
    s.close()


def _take(s, call):
    a, d = {"chunk": s.next_chunk, "row": lambda: s.next_chunk_row(0), "rows": lambda: s.next_chunks()[0]}[call]()
    return (None if a is None else a.samples), d


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_one_position_under_every_entry(gm, mode):
    """A row has one streaming position that every chunk entry follows. One row, limit 23, chunk 7 (the last chunk is the 2-frame
    remainder): twin A is read through q3_session_next_chunk alone, twin B through next_chunk, next_chunk_row(0), next_chunks(),
    next_chunk in turn — the same (samples, done) sequence, and in stream mode 1 the whole decode. While q3_session_next_chunk
    kept a position of its own beside the row's, twin B delivered frames 0-6 a second time when it changed calls.
    Parking row 0 between chunk 1 and chunk 2 is refused (a row's stream position does not travel with its record): the same
    refusal whichever entry took the first chunk, and the rows stream on unharmed."""
    opts = q.SynthesisOptions(max_length=23, seed=42, eos_token_id=None, chunk_frames=7)
    a = _session(gm, _utts([23]), opts, mode); b = _session(gm, _utts([23]), opts, mode)
    want = [_take(a, "chunk") for _ in range(4)]
    got = [_take(b, call) for call in ("chunk", "row", "rows", "chunk")]
    _same_rounds([[g] for g in got], [[w] for w in want])
    assert [len(x) // SPF for x, _ in got] == [7, 7, 7, 2] and [d for _, d in got] == [False, False, False, True]
    assert _take(a, "chunk") == (None, True) and _take(b, "row") == (None, True)
    if mode == 1:
        np.testing.assert_array_equal(np.concatenate([x for x, _ in got]), b.decode(0))
    a.close(); b.close()

    refusal = "q3_session_park_row: row 0 has delivered chunks (q3_session_next_chunk*): its stream position does not travel"
    for first in ("chunk", "row"):
        s = _session(gm, _utts([23]), opts, mode)
        got = [_take(s, first)]
        with pytest.raises(_lib.Q3Error) as e:
            s.park_row(0)
        assert refusal in str(e.value), first
        got += [_take(s, "chunk") for _ in range(3)]
        _same_rounds([[g] for g in got], [[w] for w in want])
        s.close()
