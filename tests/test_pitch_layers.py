"""A pitch per row through every layer that streams: the session (q3_session_set_pitch / _next_chunks_out), the
batcher's streamed tickets (q3_batcher_ticket_pitch / _read_out, a slot's next owner and a parked ticket included) and the CLI.
Everywhere the stream must be, bit for bit, the one-shot stage (api.resample_gpu with pitch_cents) applied to the 24 kHz f32 PCM
the same path delivers without it; rows and tickets at 0 cents must be what they are without any pitch call. Tiny synthetic model
(q.tiny())."""
import wave

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session

pytestmark = pytest.mark.gpu
PARKED = 5


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def one_shot(pcm, rate=24000, s16=False, tempo=1000, cents=0):
    return api.resample_gpu(pcm, rate, pcm16=s16, tempo_permille=tempo, pitch_cents=cents).samples


# ---------------------------------------------------------------- session
def test_session_set_pitch(gm):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 16 kHz s16; row 0 at +200 cents, row 1 at 0, row 2 at tempo 800 and -300;
    row 0 is replaced when it ends and the new utterance runs at 1250 and +386 (the pitch step alone). Every row's chunks
    concatenate to the one-shot stage on the row's next_chunks PCM from a twin session; row 1 is, chunk for chunk, that of a
    session that never heard of a pitch."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)

    def run(kind):
        s = _session(gm, limits, opts, 1)
        if kind != "pcm":
            s.set_output(16000, pcm16=True)
        if kind == "pitch":
            for bad in ((1201, 0), (-1201, -1), (200, 3)):
                with pytest.raises(_lib.Q3Error) as e:
                    s.set_pitch(*bad)
                assert e.value.status == Q3_INVALID_ARG
            s.set_pitch(-100)                              # every row ...
            s.set_pitch(200, 0); s.set_pitch(0, 1); s.set_tempo(800, 2); s.set_pitch(-300, 2)      # ... and each its own
            with pytest.raises(_lib.Q3Error) as e:
                s.set_tempo(2000)                          # row 2's pitch does not admit it (2378): no row changes
            assert e.value.status == Q3_INVALID_ARG
            with pytest.raises(_lib.Q3Error) as e:
                s.set_pitch(1200, 2)                       # nor does its tempo admit this (400)
            assert e.value.status == Q3_INVALID_ARG
        parts = {"old": [], "new": [], 1: [], 2: []}
        key = "old"; first = True
        for _ in range(32):
            r = s.next_chunks() if kind == "pcm" else s.next_chunks_out()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else b].append(a.samples)
            if first and kind == "pitch":
                for b in (0, 2, -1):                       # every row has delivered its first chunk: the setting is fixed
                    with pytest.raises(_lib.Q3Error) as e:
                        s.set_pitch(100, b)
                    assert e.value.status == Q3_INVALID_ARG
            first = False
            if r[0][1] and key == "old":
                s.replace(0, new); key = "new"
                if kind == "pitch":
                    s.set_pitch(0, 0); s.set_tempo(1250, 0); s.set_pitch(386, 0)      # the replaced row has delivered nothing yet
            elif all(d for _, d in r):
                break
        s.close()
        return parts
    got, want, plain = run("pitch"), run("pcm"), run("plain")
    pcm = {k: np.concatenate(v) for k, v in want.items()}
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 12 * SPF and pcm[2].size == 25 * SPF
    setting = {"old": (1000, 200), "new": (1250, 386), 1: (1000, 0), 2: (800, -300)}
    for k, (t, c) in setting.items():
        g = np.concatenate(got[k])
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, one_shot(pcm[k], 16000, True, t, c), err_msg=str(k))
    assert not np.array_equal(np.concatenate(got["old"]), one_shot(pcm["old"], 16000, True))
    assert len(got[1]) == len(plain[1])
    for a, w in zip(got[1], plain[1]):
        np.testing.assert_array_equal(a, w)


# ---------------------------------------------------------------- batcher
def _batcher(gm, slots, **kw):
    return q.Batcher(gm, slots=slots, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS), **kw)


@pytest.fixture(scope="module")
def plain(gm):
    """requests 0-3 of test_batcher_stream.py (5 / 50 / 20 / 27 frames) and their 24 kHz f32 PCM as plain streamed tickets"""
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(4)]
    b = _batcher(gm, 2)
    tickets = [b.submit_streamed(u) for u in utts]
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    for w in want:
        w.setflags(write=False)
    return utts, want


FOUR = [dict(sample_rate=16000, pcm16=True, pitch_cents=200), dict(), dict(tempo_permille=800, pitch_cents=-300),
        dict(sample_rate=16000, pcm16=True)]


def test_batcher_ticket_pitch(gm, plain):
    """Two slots: a ticket at +200 cents and 16 kHz s16 beside one without anything; then, in the slots they leave, one at tempo
    800 and -300 cents that is otherwise 24 kHz f32 and one at 16 kHz s16 and pitch 0 whose row had a pitch before it."""
    utts, want = plain
    b = _batcher(gm, 2)
    tickets = [b.submit_streamed(u, **kw) for u, kw in zip(utts, FOUR)]
    closed = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_pitch(closed, 200)                        # not a streamed ticket
    for t, bad in ((tickets[3], 1201), (tickets[2], 1200)):      # out of range; 800 at +1200 would need the stretcher at 400
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_pitch(t, bad)
        assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_tempo(tickets[2], 2000)                   # its pitch does not admit it
    assert e.value.status == Q3_INVALID_ARG
    b.step(STEP)
    for t in (tickets[0], tickets[3]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_pitch(t, 100)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[closed] = False
    got, _ = _drive(b, tickets + [closed], streamed, cap=1000)
    for i, t in enumerate(tickets):
        kw = FOUR[i]
        ref = one_shot(want[i], kw.get("sample_rate", 24000), kw.get("pcm16", False), kw.get("tempo_permille", 1000), kw.get("pitch_cents", 0)) if kw else want[i]
        assert b.poll(t)[0] == q.Batcher.DONE
        g = _cat(got[t])
        assert g.dtype == ref.dtype, i
        np.testing.assert_array_equal(g, ref, err_msg=f"request {i}")
    assert _cat(got[tickets[2]]).size == api.pcm_stage_pitch_count(800, -300, LIMITS[2] * SPF, True)
    b.close()


def test_a_parked_and_resumed_ticket_equals_the_uninterrupted_one(gm, plain):
    """The ticket is parked in slot 0 and goes on in slot 1: its stage row, the pitch step's tail included, follows it."""
    utts, want = plain

    def run(park):
        b = _batcher(gm, 2, **(dict(max_parked=2) if park else {}))
        S = b.submit_streamed(utts[1], pitch_cents=-300)                   # 50 frames
        b.submit(utts[0], want_pcm=False)                                  # 5 frames, row 1
        got = []
        b.step(STEP)
        a, _d = b.read(S); got.append(a)
        if park:
            b.park(S)
            assert b.poll(S)[0] == PARKED
            b.submit(utts[2], want_pcm=False)                              # takes row 0
            b.step(1)
            b.unpark(S)
            b.step(1)
            assert b.poll(S)[0] == q.Batcher.RUNNING
        for _ in range(400):
            running, queued, _f = b.step(STEP)
            a, _d = b.read(S)
            if a.size:
                got.append(a)
            if running == 0 and queued == 0:
                break
        a, done = b.read(S); got.append(a)
        assert done
        if park:
            assert b.park_info()["moved"] == 1
        b.close()
        return _cat([x for x in got if x.size])

    ref, got = run(False), run(True)
    np.testing.assert_array_equal(ref.view(np.uint32), one_shot(want[1], cents=-300).view(np.uint32))
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))


# ---------------------------------------------------------------- CLI
def test_cli_pitch(tmp_path):
    args = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7"]
    out = tmp_path / "o"
    assert cli.main(args + ["--output-dir", str(out), "--streaming", "--pitch", "2"]) == 0
    with wave.open(str(out / "audio_seed7_frames9.wav")) as w:
        assert (w.getnframes(), w.getframerate(), w.getsampwidth()) == (api.pcm_stage_pitch_count(1000, 200, 9 * SPF, True), 24000, 2)
    assert cli.main(args + ["--output-dir", str(tmp_path / "o2"), "--streaming"]) == 0
    pcm24 = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    np.testing.assert_array_equal(np.fromfile(out / "audio_seed7_frames9.bin", dtype="<f4"), one_shot(pcm24, cents=200))
    assert cli.main(args + ["--output-dir", str(tmp_path / "o3"), "--pitch", "2"]) == 2                      # not without --streaming
    assert cli.main(args + ["--output-dir", str(tmp_path / "o3"), "--streaming", "--pitch", "12.5"]) == 2
    assert cli.main(args + ["--output-dir", str(tmp_path / "o3"), "--streaming", "--tempo", "2.0", "--pitch", "-3"]) == 2
