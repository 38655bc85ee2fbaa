"""Streaming text input: a row opened before the prefill takes the rest of its text in pieces while it speaks.
Frame f of a row depends on the text only through trailing token f, so a row whose frames are HELD while their token is
missing must give the codes (and PCM) of the same request with its whole text, bit for bit, under any feeding schedule."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt

NEW = ["q3_session_open_text", "q3_session_append_text", "q3_session_text_state"]


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.lib.q3_abi_version() == 1


def test_null_handles_and_bad_arguments_return_status():
    L = _lib.lib
    i = ctypes.c_int()
    ids = (ctypes.c_uint32 * 2)(1, 2)
    calls = [
        lambda: L.q3_session_open_text(None, 0),
        lambda: L.q3_session_append_text(None, 0, ids, 2, 0),
        lambda: L.q3_session_append_text(None, 0, None, 3, 1),
        lambda: L.q3_session_text_state(None, 0, ctypes.byref(i), None, None, None, None),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error()


def test_python_surface():
    assert callable(api.Session.open_text) and callable(api.Session.append_text) and callable(api.Session.text_state)
    assert callable(q.Qwen3TTS.synthesize_streaming_text)
    for m in ("push", "finish", "next_chunk", "is_done"):
        assert callable(getattr(q.TextStreamingSession, m)), m


# ---------------------------------------------------------------- tiny model on the GPU
PATHS = ["aql", "hipgraph", "eager"]


def _path(monkeypatch, path):
    """frame submission path: own AQL queue (default), hipGraphLaunch (Q3_AQL=0, read per session), eager launches"""
    if path == "hipgraph":
        monkeypatch.setenv("Q3_AQL", "0")
    else:
        monkeypatch.delenv("Q3_AQL", raising=False)
    return path != "eager"


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def _opts(sampling, L):
    if sampling == "greedy":
        return q.SynthesisOptions(max_length=L, temperature=0.0, seed=42, eos_token_id=None)
    return q.SynthesisOptions(max_length=L, seed=42, eos_token_id=None)


def _closed(gm, utts, opts, use_graph, L, **kw):
    s = gm.session(utts, opts, **kw); s.prefill(); s.generate(L, use_graph=use_graph)
    out = [(s.codes(b), s.decode(b)) for b in range(len(utts))]
    s.close()
    return out


def _first(u, k):
    v = api.Utterance(**{f: getattr(u, f) for f in u.__dataclass_fields__})
    v.text_ids = list(u.text_ids)[:k]
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("sampling", ["greedy", "seeded"])
def test_one_token_per_generate_equals_closed(gm, monkeypatch, path, sampling):
    use_graph = _path(monkeypatch, path)
    L = 24
    full = synthetic_prompt(12, 0)
    u = q.Utterance(full, q.Speaker.Ryan, q.Language.English, seed=42)
    opts = _opts(sampling, L)
    (ref_codes, ref_pcm), = _closed(gm, [u], opts, use_graph, L)
    s = gm.session([_first(u, 1)], opts); s.open_text(0); s.prefill()
    st = s.text_state(0)
    assert st["n_text"] == 1 and st["frames_committed"] == 0 and not st["closed"]
    for i in range(1, len(full)):
        s.append_text(0, [full[i]])
        s.generate(3, use_graph=use_graph)
        st = s.text_state(0)
        assert st["n_text"] == i + 1
        assert st["frames_committed"] <= i, (i, st)           # one committed frame per trailing token received at most
        assert st["frames_committed"] == i and st["frames_runnable"] == 0, (i, st)      # ... and held at the first missing one
    s.append_text(0, [], last=True)
    assert s.text_state(0)["closed"]
    with pytest.raises(_lib.Q3Error):
        s.append_text(0, [full[0]])                           # an append after the close
    s.generate(L, use_graph=use_graph)
    codes = s.codes(0)
    np.testing.assert_array_equal(codes, ref_codes)
    np.testing.assert_array_equal(s.decode(0), ref_pcm)
    s.close()


def _mixed4(L):
    utts = [q.Utterance(synthetic_prompt(n, i), q.Speaker.Ryan, q.Language.English, seed=100 + i) for i, n in enumerate((9, 14, 17, 1))]
    return utts


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_mixed_schedules_b4(gm, monkeypatch, path):
    """row 0 closed from the start; row 1 a token every 3 frames; row 2 in bursts; row 3 closed after its single token"""
    use_graph = _path(monkeypatch, path)
    L = 22
    utts = _mixed4(L)
    opts = _opts("seeded", L)
    ref = _closed(gm, utts, opts, use_graph, L)
    first = [utts[0], _first(utts[1], 1), _first(utts[2], 3), _first(utts[3], 1)]
    s = gm.session(first, opts)
    for b in (1, 2, 3):
        s.open_text(b)
    s.prefill()
    fed = [None, 1, 3, 1]
    for it in range(200):
        if it % 3 == 0 and fed[1] is not None:
            k = fed[1]; t = list(utts[1].text_ids)
            if k < len(t):
                s.append_text(1, [t[k]]); fed[1] += 1
            else:
                s.append_text(1, [], last=True); fed[1] = None
        if it % 7 == 2 and fed[2] is not None:
            k = fed[2]; t = list(utts[2].text_ids)
            s.append_text(2, t[k:k + 5], last=k + 5 >= len(t)); fed[2] = None if k + 5 >= len(t) else k + 5
        if it == 1:
            s.append_text(3, [], last=True)
        s.generate(1, use_graph=use_graph)
        if all(s.frames(b)[1] for b in range(4)):
            break
    for b in range(4):
        assert s.text_state(b)["frames_committed"] == L, (b, s.text_state(b))
        np.testing.assert_array_equal(s.codes(b), ref[b][0], err_msg=f"row {b}")
        np.testing.assert_array_equal(s.decode(b), ref[b][1], err_msg=f"row {b} PCM")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_held_session_replays_nothing(gm, monkeypatch, path):
    use_graph = _path(monkeypatch, path)
    L = 16
    utts = [q.Utterance(synthetic_prompt(10, 7 + i), q.Speaker.Ryan, q.Language.English, seed=7 + i) for i in range(2)]
    opts = _opts("seeded", L)
    ref = _closed(gm, utts, opts, use_graph, L)
    s = gm.session([_first(u, 1) for u in utts], opts)
    s.open_text(0); s.open_text(1); s.prefill()
    s.generate(100, use_graph=use_graph)
    st = [s.text_state(b) for b in range(2)]
    assert st[0]["frames_replayed"] == 0 and st[0]["frames_committed"] == 0 and st[1]["frames_committed"] == 0, st
    t0 = list(utts[0].text_ids)
    s.append_text(0, t0[1:4])                                  # row 0 can commit exactly 3 more frames
    assert s.text_state(0)["frames_runnable"] == 3
    s.generate(100, use_graph=use_graph)
    st = [s.text_state(b) for b in range(2)]
    assert st[0]["frames_replayed"] == 3 and st[0]["frames_committed"] == 3 and st[1]["frames_committed"] == 0, st
    s.generate(100, use_graph=use_graph)
    assert s.text_state(0)["frames_replayed"] == 3
    s.append_text(0, t0[4:], last=True); s.append_text(1, list(utts[1].text_ids)[1:], last=True)
    s.generate(100, use_graph=use_graph)
    for b in range(2):
        np.testing.assert_array_equal(s.codes(b), ref[b][0], err_msg=f"row {b}")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("path", ["aql", "hipgraph"])
@pytest.mark.parametrize("continuous", [False, True])
@pytest.mark.parametrize("chunk", [2, 10])
def test_streaming_text_equals_closed_streaming(gm, monkeypatch, path, continuous, chunk):
    _path(monkeypatch, path)
    L = 23
    full = synthetic_prompt(15, 3)
    opts = q.SynthesisOptions(max_length=L, seed=5, eos_token_id=None, chunk_frames=chunk)
    ref = gm.synthesize_streaming(full, q.Speaker.Ryan, q.Language.English, opts, continuous=continuous)
    ref_chunks = [c.samples for c in ref]
    ref_codes = ref._s.codes(0)
    ts = gm.synthesize_streaming_text(full[:1], q.Speaker.Ryan, q.Language.English, opts, continuous=continuous)
    got, waits = [], 0
    for tok in full[1:]:
        ts.push([tok])
        c = ts.next_chunk()
        if c is None:
            waits += 1
        else:
            got.append(c.samples)
    ts.finish()
    while not ts.is_done():
        c = ts.next_chunk()
        assert c is not None or ts.is_done()
        if c is not None:
            got.append(c.samples)
    assert waits > 0                                           # next_chunk really waited for text
    assert [len(g) for g in got] == [len(r) for r in ref_chunks]
    np.testing.assert_array_equal(np.concatenate(got), np.concatenate(ref_chunks))
    np.testing.assert_array_equal(ts._s.codes(0), ref_codes)
    ts.close()


def _feed_token_by_token(s, b, t, use_graph):
    for tok in t:
        s.append_text(b, [tok])
        s.generate(2, use_graph=use_graph)
    s.append_text(b, [], last=True)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["design", "xvector", "icl", "bf16"])
def test_more_session_kinds(gm, kind):
    cfg = gm.config
    L = 20
    rng = np.random.default_rng(11)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)
    opts = _opts("seeded", L)
    kw = {}
    if kind == "design":
        u = q.Utterance(synthetic_prompt(11, 1), language=q.Language.German, instruct_ids=synthetic_prompt(7, 51), seed=43)
    elif kind == "xvector":
        u = q.Utterance(synthetic_prompt(11, 2), language=q.Language.French, xvector=xv, seed=44)
    elif kind == "icl":
        ref = rng.integers(0, 2048, size=(5, 16)).astype(np.uint32)
        u = q.Utterance(synthetic_prompt(14, 4), language=q.Language.French, xvector=xv, ref_codes=ref,
                        ref_text_ids=synthetic_prompt(3, 94), seed=46)
        opts = q.SynthesisOptions(max_length=L, seed=42, eos_token_id=None)
    else:
        u = q.Utterance(synthetic_prompt(11, 3), q.Speaker.Ryan, q.Language.English, seed=45)
        kw = {"kv_bf16": True}
    (ref_codes, ref_pcm), = _closed(gm, [u], opts, True, L, **kw)
    k0 = 3 if kind == "icl" else 1                            # ICL: n_ref + 1 - n_ref_text = 3 target tokens at creation
    if kind == "icl":
        s = gm.session([_first(u, k0 - 1)], opts)
        with pytest.raises(_lib.Q3Error, match="ICL"):
            s.open_text(0)                                     # too few: tts_eos would fall inside the ICL block
        s.close()
    s = gm.session([_first(u, k0)], opts, **kw); s.open_text(0); s.prefill()
    _feed_token_by_token(s, 0, list(u.text_ids)[k0:], True)
    s.generate(L, use_graph=True)
    np.testing.assert_array_equal(s.codes(0), ref_codes)
    np.testing.assert_array_equal(s.decode(0), ref_pcm)
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("B", [20, 33])
def test_wide_sessions(gm, B):
    L = 12
    utts = [q.Utterance(synthetic_prompt(8 + i % 5, i), q.Speaker.Ryan, q.Language.English, seed=200 + i) for i in range(B)]
    opts = _opts("seeded", L)
    ref = _closed(gm, utts, opts, True, L)
    opened = [1, B // 2, B - 1]
    s = gm.session([_first(u, 1) if b in opened else u for b, u in enumerate(utts)], opts)
    for b in opened:
        s.open_text(b)
    s.prefill()
    pos = {b: 1 for b in opened}
    for it in range(60):
        for j, b in enumerate(opened):
            t = list(utts[b].text_ids)
            if pos[b] is not None and it % (j + 2) == 0:
                if pos[b] < len(t):
                    s.append_text(b, [t[pos[b]]]); pos[b] += 1
                else:
                    s.append_text(b, [], last=True); pos[b] = None
        s.generate(1, use_graph=True)
        if all(s.frames(b)[1] for b in range(B)):
            break
    for b in sorted(set(opened + [0, B - 2])):
        np.testing.assert_array_equal(s.codes(b), ref[b][0], err_msg=f"row {b}")
    s.close()


@pytest.mark.gpu
def test_refusals(gm):
    opts = _opts("seeded", 8)
    u = q.Utterance(synthetic_prompt(5, 1), q.Speaker.Ryan, q.Language.English, seed=1)
    s = gm.session([u, u], opts)
    with pytest.raises(_lib.Q3Error, match="not open"):
        s.append_text(0, [1])
    s.open_text(0)
    with pytest.raises(_lib.Q3Error, match="still open"):
        s.run()
    s.prefill()
    with pytest.raises(_lib.Q3Error, match="before q3_session_prefill"):
        s.open_text(1)
    s.close()
    s = gm.session([u], opts, debug=True)
    with pytest.raises(_lib.Q3Error, match="debug"):
        s.open_text(0)
    s.close()
    s = gm.session([u, q.Utterance(synthetic_prompt(5, 2), language=q.Language.German, instruct_ids=synthetic_prompt(4, 3), seed=2)], opts)
    with pytest.raises(_lib.Q3Error, match="ragged"):
        s.open_text(0)
    s.close()


@pytest.mark.gpu
def test_replace_open_row_and_append_after_end(gm):
    L = 10
    opts = _opts("seeded", L)
    u = q.Utterance(synthetic_prompt(9, 4), q.Speaker.Ryan, q.Language.English, seed=9)
    (ref_codes, _), = _closed(gm, [u], opts, True, L)
    s = api.Session(gm, [_first(u, 1)], opts, frame_budget=L)
    s.open_text(0); s.prefill()
    s.append_text(0, list(u.text_ids)[1:4])
    s.generate(L)
    s.replace(0, u)                                            # an ordinary closed request in the open row
    s.generate(L)
    np.testing.assert_array_equal(s.codes(0), ref_codes)
    s.close()
    short = q.SynthesisOptions(max_length=2, seed=42, eos_token_id=None)
    s = gm.session([_first(u, 4)], short); s.open_text(0); s.prefill(); s.generate(10)
    assert s.frames(0) == (2, True)
    s.append_text(0, [5, 6, 7])                                # the row has ended: accepted, ignored
    s.append_text(0, [], last=True)
    assert s.frames(0) == (2, True)
    s.close()


@pytest.mark.gpu
def test_cli_feed_tokens_writes_the_same_wav(tmp_path, capsys):
    from qwen3_tts_rs_amd import cli
    ids = ",".join(str(int(x)) for x in synthetic_prompt(9, 2))
    base = ["--synthetic", "tiny", "--token-ids", ids, "--frames", "14", "--no-eos", "--seed", "7"]
    assert cli.main(base + ["--output-dir", str(tmp_path / "a"), "--output", str(tmp_path / "a.wav")]) == 0
    assert cli.main(base + ["--feed-tokens", "2", "--output-dir", str(tmp_path / "b"), "--output", str(tmp_path / "b.wav")]) == 0
    assert "first token to first audio" in capsys.readouterr().out
    assert open(tmp_path / "a.wav", "rb").read() == open(tmp_path / "b.wav", "rb").read()


# ---------------------------------------------------------------- 1.7B (synthetic weights)
@pytest.fixture(scope="module")
def gm17():
    from qwen3_tts_rs_amd import synth
    m = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    yield m
    m.close()


@pytest.mark.gpu
def test_1_7b_trailing_rows_and_codes_independent_of_feeding(gm17):
    """Appended tokens take one projection path: their rows — and so the codes — are bit-identical whether the text came token
    by token between frames or in one append (at 1.7B the prompt projection's GEMM and GEMV sum in different orders)."""
    cfg = gm17.config
    L = 40
    full = synthetic_prompt(120, 0)
    u = q.Utterance(full, q.Speaker.Ryan, q.Language.English, seed=42)
    opts = q.SynthesisOptions(max_length=L, seed=42, eos_token_id=None)
    a = gm17.session([_first(u, 1)], opts); a.open_text(0); a.prefill()
    b = gm17.session([_first(u, 1)], opts); b.open_text(0); b.prefill()
    b.append_text(0, full[1:60])                               # all at once (closed below with the rest)
    for i in range(1, len(full)):
        a.append_text(0, [full[i]])
        if i < 12:
            a.generate(1)                                      # (the row stays short of its limit: appends to an ended row are ignored)
    _, ta = a.prefill_len(0); _, tb = b.prefill_len(0)
    assert ta == len(full) - 1 and tb == 59
    ra = a.get(3, (ta, cfg.hidden))
    b.append_text(0, full[60:])
    rb = b.get(3, (ta, cfg.hidden))
    np.testing.assert_array_equal(ra, rb)
    a.append_text(0, [], last=True); b.append_text(0, [], last=True)
    a.generate(L); b.generate(L)
    np.testing.assert_array_equal(a.codes(0), b.codes(0))
    assert a.codes(0).shape == (L, 16)
    a.close(); b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("sampling", ["greedy", "default"])
def test_1_7b_b8_fed_in_pieces_matches_fixture(gm17, sampling):
    """The benchmark's eight 512-token prompts (seeds 42 + i, tests/golden/bench_1_7b_codes.npz) opened with a few tokens each and
    fed in irregular pieces between frames: every row's codes equal the oracle fixture. A divergence is tolerated only at an
    oracle near-tie (adjudicated live as in test_bench_config_parity), at most one per eight sequences."""
    import os
    from make_golden_bench import bench_utt, N_FRAMES
    from test_bench_config_parity import _adjudicate
    B = 8
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_1_7b_codes.npz"))[f"{sampling}_codes"]
    kw = dict(temperature=0.0) if sampling == "greedy" else {}
    opts = q.SynthesisOptions(max_length=N_FRAMES, eos_token_id=None, seed=42, **kw)
    utts = [bench_utt(i) for i in range(B)]
    pos = [1 + (3 * b) % 5 for b in range(B)]
    s = gm17.session([_first(u, pos[b]) for b, u in enumerate(utts)], opts)
    for b in range(B):
        s.open_text(b)
    s.prefill()
    held = 0
    for it in range(4 * N_FRAMES):
        for b in range(B):
            k = (it * 7 + b * 3) % 5 if (it + b) % 3 else 0          # 0 .. 4 tokens, some steps none
            t = list(utts[b].text_ids)
            if k and pos[b] < len(t):
                s.append_text(b, t[pos[b]:pos[b] + k]); pos[b] += k
        s.generate(1)
        held += sum(1 for b in range(B) if s.text_state(b)["frames_runnable"] == 0 and not s.frames(b)[1])
        if all(s.frames(b)[1] for b in range(B)):
            break
    assert held > 0                                                 # rows really waited for text
    report = []
    for b, u in enumerate(utts):
        codes = s.codes(b)
        assert codes.shape == ref[b].shape, (b, codes.shape)
        if not (codes == ref[b]).all():
            ok, rep = _adjudicate("1.7b", u, opts, codes, f"1_7b_b8_{sampling}_open_text_seq{b}")
            report.append(rep)
            assert ok, rep
    s.close()
    assert len(report) <= 1, report
