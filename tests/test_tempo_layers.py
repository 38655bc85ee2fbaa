"""A speaking rate per row through every layer that streams: the codec stream (q3_codec_stream_push_out through a
stage row with a tempo), the session (q3_session_set_tempo / _next_chunks_out), the batcher's streamed tickets
(q3_batcher_ticket_tempo / _read_out) and the CLI. Everywhere the stream must be, bit for bit, the one-shot stage
(api.resample_gpu with tempo_permille) applied to the 24 kHz f32 PCM the same path delivers without it; rows and tickets at 1000
must be what they are without any tempo call. Tiny synthetic model (q.tiny())."""
import wave

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session, _rounds


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def one_shot(pcm, rate, s16, tempo=1000):
    return api.resample_gpu(pcm, rate, pcm16=s16, tempo_permille=tempo).samples


def n_out(n, t):
    return (n * 1000 + t // 2) // t


# ---------------------------------------------------------------- codec stream
@pytest.mark.gpu
def test_codec_stream_push_out_with_tempo(gm):
    """40 random frames to two rows in pieces 1, 2, 9, 13, 15: row 0 at 16 kHz s16 and 1250, row 1 at 24 kHz f32 and 800; then
    the same rows at 1000 on the same stage: the bits of a stage that never had a tempo."""
    rng = np.random.default_rng(5)
    codes = {r: rng.integers(0, 2048, size=(40, 16)).astype(np.uint32) for r in (0, 1)}
    whole = {r: gm.decode_codes(codes[r]).samples.copy() for r in (0, 1)}
    fmt = {0: (16000, True), 1: (24000, False)}
    pieces = [1, 2, 9, 13, 15]

    def run(ps, tempo):
        cs = gm.codec_stream(2, 40)
        for r in (0, 1):
            ps.set(r, *fmt[r])
            if tempo is not None:
                ps.set_tempo(r, tempo[r])
        got = {0: [], 1: []}; at = 0
        for k, n in enumerate(pieces):
            out = cs.push({r: codes[r][at:at + n] for r in (0, 1)}, stage=ps, last=(0, 1) if k == len(pieces) - 1 else ())
            at += n
            for r in (0, 1):
                got[r].append(out[r])
                assert cs.pos(r) == at
        cs.close()
        return {r: np.concatenate(got[r]) for r in (0, 1)}
    ps = gm.pcm_stage(2, 40 * SPF)
    tempo = {0: 1250, 1: 800}
    g = run(ps, tempo)
    for r in (0, 1):
        assert g[r].dtype == (np.int16 if fmt[r][1] else np.float32)
        np.testing.assert_array_equal(g[r], one_shot(whole[r], *fmt[r], tempo[r]), err_msg=f"row {r}")
    assert g[1].size == n_out(40 * SPF, 800)
    k0, lags = ps.tempo_lags(0)
    assert lags.size > 0 and k0 + lags.size == -(-n_out(40 * SPF, 1250) // 360)
    back = run(ps, {0: 1000, 1: 1000})
    plain = gm.pcm_stage(2, 40 * SPF)
    want = run(plain, None)
    for r in (0, 1):
        np.testing.assert_array_equal(back[r], want[r], err_msg=f"row {r} at 1000")
    np.testing.assert_array_equal(want[1], whole[1])
    ps.close(); plain.close()


# ---------------------------------------------------------------- session
@pytest.mark.gpu
def test_session_set_tempo(gm):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 16 kHz s16, tempos 1250 / 1000 / 500; row 0 is replaced when it ends
    and the new utterance runs at 2000. Every row's chunks concatenate to the one-shot stage on the row's next_chunks PCM from a
    twin session; row 1 is, chunk for chunk, that of a session that never heard of a tempo."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)

    def run(kind):
        s = _session(gm, limits, opts, 1)
        if kind != "pcm":
            s.set_output(16000, pcm16=True)
        if kind == "tempo":
            with pytest.raises(_lib.Q3Error) as e:
                s.set_tempo(2001, 0)
            assert e.value.status == Q3_INVALID_ARG
            with pytest.raises(_lib.Q3Error):
                s.set_tempo(1250, 3)                       # no such row
            s.set_tempo(800)                               # every row ...
            s.set_tempo(1250, 0); s.set_tempo(1000, 1); s.set_tempo(500, 2)      # ... and each its own
        parts = {"old": [], "new": [], 1: [], 2: []}
        key = "old"; first = True
        for _ in range(32):
            r = s.next_chunks() if kind == "pcm" else s.next_chunks_out()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else b].append(a.samples)
            if first and kind == "tempo":
                # every row has delivered its first chunk: the setting is fixed, for one row and for all
                for b in (0, 2, -1):
                    with pytest.raises(_lib.Q3Error) as e:
                        s.set_tempo(1500, b)
                    assert e.value.status == Q3_INVALID_ARG
            first = False
            if r[0][1] and key == "old":
                s.replace(0, new); key = "new"
                if kind == "tempo":
                    s.set_tempo(2000, 0)                   # the replaced row has delivered nothing yet
            elif all(d for _, d in r):
                break
        s.close()
        return parts
    got, want, plain = run("tempo"), run("pcm"), run("plain")
    pcm = {k: np.concatenate(v) for k, v in want.items()}
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 12 * SPF and pcm[2].size == 25 * SPF
    tempo = {"old": 1250, "new": 2000, 1: 1000, 2: 500}
    for k, t in tempo.items():
        g = np.concatenate(got[k])
        assert g.dtype == np.int16
        assert g.size == int(np.floor(n_out(pcm[k].size, t) * (16000 / 24000.0) + 0.5)), k
        np.testing.assert_array_equal(g, one_shot(pcm[k], 16000, True, t), err_msg=str(k))
    assert len(got[1]) == len(plain[1])
    for a, w in zip(got[1], plain[1]):
        np.testing.assert_array_equal(a, w)


@pytest.mark.gpu
def test_session_tempo_is_ignored_by_the_other_calls(gm):
    """next_chunks with a tempo set: the 24 kHz f32 chunks of a session without one (as q3_session_set_output is ignored)."""
    limits = [7, 12]
    opts = q.SynthesisOptions(max_length=12, seed=42, eos_token_id=None, chunk_frames=5)
    s = _session(gm, limits, opts, 1); t = _session(gm, limits, opts, 1)
    s.set_tempo(1250)
    got, _ = _rounds(s, False); want, _ = _rounds(t, False)
    for b in range(2):
        np.testing.assert_array_equal(np.concatenate([a.samples for a in got[b]]), np.concatenate([a.samples for a in want[b]]))
    s.close(); t.close()


# ---------------------------------------------------------------- batcher
FOUR = [(16000, True, 1250), (24000, False, 1000), (24000, False, 800), (16000, True, 1000)]


@pytest.mark.gpu
def test_batcher_ticket_tempo(gm):
    """Requests 0-3 of test_batcher_stream.py (5 / 50 / 20 / 27 frames) through two slots: a ticket at 1250 and 16 kHz s16 beside
    one without anything; then, in the slots they leave, one at 800 that is otherwise 24 kHz f32 and one at 16 kHz s16 whose row
    had a tempo before it."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(4)]

    def batcher():
        return q.Batcher(gm, slots=2, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    b = batcher()
    tickets = [b.submit_streamed(u) for u in utts]
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    b = batcher()
    tickets = [b.submit_streamed(u, sample_rate=sr, pcm16=s16, tempo_permille=t) for u, (sr, s16, t) in zip(utts, FOUR)]
    plain = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_tempo(plain, 1250)                        # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_tempo(tickets[3], 499)
    assert e.value.status == Q3_INVALID_ARG
    b.step(STEP)
    for t in (tickets[0], tickets[3]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_tempo(t, 1500)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[plain] = False
    got, _ = _drive(b, tickets + [plain], streamed, cap=1000)
    for i, t in enumerate(tickets):
        sr, s16, tp = FOUR[i]
        g = _cat(got[t])
        assert g.dtype == (np.int16 if s16 else np.float32), i
        assert b.poll(t)[0] == q.Batcher.DONE
        np.testing.assert_array_equal(g, one_shot(want[i], sr, s16, tp) if (sr, s16, tp) != (24000, False, 1000) else want[i], err_msg=f"request {i}")
    assert _cat(got[tickets[2]]).size == n_out(LIMITS[2] * SPF, 800)
    b.close()


# ---------------------------------------------------------------- CLI
@pytest.mark.gpu
def test_cli_tempo(tmp_path):
    out = tmp_path / "o"
    rc = cli.main(["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7",
                   "--output-dir", str(out), "--streaming", "--tempo", "1.25"])
    assert rc == 0
    with wave.open(str(out / "audio_seed7_frames9.wav")) as w:
        assert (w.getnframes(), w.getframerate(), w.getsampwidth()) == (n_out(9 * SPF, 1250), 24000, 2)
    rc = cli.main(["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7",
                   "--output-dir", str(tmp_path / "o2"), "--streaming"])
    assert rc == 0
    pcm24 = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    np.testing.assert_array_equal(np.fromfile(out / "audio_seed7_frames9.bin", dtype="<f4"), one_shot(pcm24, 24000, False, 1250))
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3"), "--tempo", "1.25"]) == 2
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3"), "--streaming", "--tempo", "2.5"]) == 2
