"""The loudness step through every layer that streams: the session (q3_session_set_loudness / _loudness /
_next_chunks_out), the batcher's streamed tickets (q3_batcher_ticket_loudness / _loudness_read / _read_out, parked tickets
included) and api.loudness. Everywhere the stream and the reading must be, bit for bit, those of the one-shot stage applied to the
24 kHz f32 PCM the same path delivers without the step. Tiny synthetic model (q.tiny())."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session
from test_loudness_host import GOLDEN, TOL_LU, make_signal

pytestmark = pytest.mark.gpu
OFF, METER, NORM = api.LOUD_OFF, api.LOUD_METER, api.LOUD_NORMALIZE
PARKED = 5


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def one_shot(pcm, rate=24000, fmt="f32", loud=(OFF, -1900, 0), level=(0, 0)):
    """(samples, reading) of the one-shot stage; the reading is None for a row whose step is off"""
    ps = api.PcmStage(0, 1, max(pcm.size, 1))
    try:
        ps.set(0, rate, fmt=fmt); ps.set_level(0, *level); ps.set_loudness(0, *loud)
        out = ps.push({0: pcm}, last=(0,))[0]
        return out, (ps.loudness(0) if loud[0] != OFF else None)
    finally:
        ps.close()


# ---------------------------------------------------------------- session
def test_session_loudness_window_and_replace(gm):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 16 kHz s16; row 0 normalises to -1900 from +600, row 1 has no step, row 2
    meters behind a setting for every row that was then changed. Row 0 is replaced when it ends: the new utterance keeps the row's
    setting and starts the row over. Every row's chunks concatenate to the one-shot stage on the row's next_chunks PCM from a twin
    session, and its reading is that stage's. After the first streamed chunk the setting is fixed."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)
    loud = {"old": (NORM, -1900, 600), "new": (NORM, -1900, 600), 1: (OFF, -1900, 0), 2: (METER, -2300, 0)}
    readings = {}

    def run(kind):
        s = _session(gm, limits, opts, 1)
        if kind == "out":
            s.set_output(16000, pcm16=True)
            for bad in ((3, -1900, 0, 0), (NORM, -499, 0, 0), (NORM, -1900, 2401, 0), (NORM, -1900, 0, 3)):
                with pytest.raises(_lib.Q3Error) as e:
                    s.set_loudness(*bad)
                assert e.value.status == Q3_INVALID_ARG
            s.set_loudness(NORM, -1600, -300)              # every row ...
            s.set_loudness(*loud["old"], 0); s.set_loudness(OFF, b=1); s.set_loudness(*loud[2], 2)      # ... and each its own
            r = s.loudness(0)
            assert r.blocks == 0 and abs(r.gain_db - 6.0) < 1e-5      # nothing streamed yet: the row stands at its prior
            with pytest.raises(_lib.Q3Error):
                s.loudness(1)                              # a row without the step has no reading
        parts = {"old": [], "new": [], 1: [], 2: []}
        key = "old"; first = True
        for _ in range(32):
            r = s.next_chunks() if kind == "pcm" else s.next_chunks_out()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else b].append(a.samples)
            if first and kind == "out":
                before = (s.loudness(0), s.loudness(2))
                for b in (0, 2, -1):                       # every row has delivered its first chunk: the setting is fixed
                    with pytest.raises(_lib.Q3Error) as e:
                        s.set_loudness(METER, -1900, 0, b)
                    assert e.value.status == Q3_INVALID_ARG
                assert (s.loudness(0), s.loudness(2)) == before      # ... and no row changed
            first = False
            if r[0][1] and key == "old":
                if kind == "out":
                    readings["old"] = s.loudness(0)
                s.replace(0, new); key = "new"
            elif all(d for _, d in r):
                break
        if kind == "out":
            readings["new"] = s.loudness(0); readings[2] = s.loudness(2)
        s.close()
        return parts
    got, want = run("out"), run("pcm")
    pcm = {k: np.concatenate(v) for k, v in want.items()}
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 12 * SPF and pcm[2].size == 25 * SPF
    for k, ld in loud.items():
        g = np.concatenate(got[k])
        ref, reading = one_shot(pcm[k], 16000, "s16", ld)
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, ref, err_msg=str(k))
        if reading is not None:
            print(f"row {k}: {reading}")
            assert readings[k] == reading, k
            assert reading.blocks == pcm[k].size // 2400 - 3
    assert readings["old"].gated > 0 and readings[2].gated > 0      # the tiny model's audio passes the gates: the step had work
    assert not np.array_equal(np.concatenate(got["new"]), one_shot(pcm["new"], 16000, "s16")[0])


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


def test_batcher_tickets_with_their_own_target_and_prior(gm, plain):
    """Two slots: a normalised ticket at 8 kHz mu-law beside a plain one; then, in the slots they leave, another target and prior at
    24 kHz f32 behind a ceiling (read through read_out) and a ticket without the step in a row that had it. The reading is final
    once `read` has reported the ticket done and stays until `fetch`."""
    utts, want = plain
    four = [dict(sample_rate=8000, fmt="ulaw", target_lufs=-19.0), dict(),
            dict(target_lufs=-23.0, prior_gain_db=6.0, ceiling_mb=-100), dict(sample_rate=16000, fmt="s16")]
    b = _batcher(gm, 2)
    tickets = [b.submit_streamed(u, **kw) for u, kw in zip(utts, four)]
    closed = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_loudness(closed, NORM, -1900, 0)          # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_loudness(tickets[3], NORM, -1900, 2401)
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error):
        b.loudness(tickets[1])                             # a ticket without the step has no reading
    assert b.loudness(tickets[2]).blocks == 0 and abs(b.loudness(tickets[2]).gain_db - 6.0) < 1e-5
    b.step(STEP)
    for t in (tickets[0], tickets[3]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_loudness(t, METER, -1900, 0)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[closed] = False
    got, _ = _drive(b, tickets + [closed], streamed, cap=1000)
    refs = [one_shot(want[0], 8000, "ulaw", (NORM, -1900, 0)), (want[1], None),
            one_shot(want[2], 24000, "f32", (NORM, -2300, 600), (0, -100)), one_shot(want[3], 16000, "s16")]
    for i, t in enumerate(tickets):
        assert b.poll(t)[0] == q.Batcher.DONE
        np.testing.assert_array_equal(_cat(got[t]), refs[i][0], err_msg=f"request {i}")
        if refs[i][1] is not None:
            print(f"request {i}: {refs[i][1]}")
            assert b.loudness(t) == refs[i][1], i          # final after `done`
    assert refs[2][1].gated > 0 and float(np.max(np.abs(refs[2][0]))) <= float(api.pcm_stage_level_coeffs(0, -100)[1])
    b.fetch(tickets[0])
    with pytest.raises(_lib.Q3Error):
        b.loudness(tickets[0])                             # released
    b.close()


def test_a_slots_next_owner_starts_from_its_own_setting(gm, plain):
    """One slot. A normalised ticket is cancelled in mid-run; the next owner of its slot (metering) and the one after (another
    target, a prior) each start from their own setting, with an empty history."""
    utts, want = plain
    b = _batcher(gm, 1)
    A = b.submit_streamed(utts[1], target_lufs=-19.0, prior_gain_db=-6.0)
    B = b.submit_streamed(utts[2]); b.ticket_loudness(B, METER)
    C = b.submit_streamed(utts[3], target_lufs=-30.0, prior_gain_db=12.0)
    b.step(STEP); b.step(STEP)
    assert b.poll(A)[0] == q.Batcher.RUNNING
    b.cancel(A)
    got, _ = _drive(b, [A, B, C], {A: True, B: True, C: True})
    n24 = b.poll(A)[1] * SPF                               # the frames A committed, flushed
    assert 0 < n24 < LIMITS[1] * SPF
    for t, ref in ((A, one_shot(want[1][:n24], loud=(NORM, -1900, -600))), (B, one_shot(want[2], loud=(METER, -1900, 0))),
                   (C, one_shot(want[3], loud=(NORM, -3000, 1200)))):
        np.testing.assert_array_equal(_cat(got[t]).view(np.uint32), ref[0].view(np.uint32))
        assert b.loudness(t) == ref[1]
    np.testing.assert_array_equal(_cat(got[B]), want[2])
    b.close()


def test_a_parked_and_resumed_ticket_equals_the_uninterrupted_one(gm, plain):
    """The ticket is parked in slot 0 and goes on in slot 1: its stage row follows it, history included."""
    utts, want = plain

    def run(park):
        b = _batcher(gm, 2, **(dict(max_parked=2) if park else {}))
        S = b.submit_streamed(utts[1], target_lufs=-19.0)                  # 50 frames
        X = b.submit(utts[0], want_pcm=False)                              # 5 frames, row 1
        got = []
        b.step(STEP)
        a, _d = b.read(S); got.append(a)
        if park:
            b.park(S)
            assert b.poll(S)[0] == PARKED
            Y = b.submit(utts[2], want_pcm=False)                          # takes row 0
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
        r = b.loudness(S)
        if park:
            assert b.park_info()["moved"] == 1
        b.close()
        return _cat([x for x in got if x.size]), r

    ref, got = run(False), run(True)
    want_one = one_shot(want[1], loud=(NORM, -1900, 0))
    np.testing.assert_array_equal(ref[0].view(np.uint32), want_one[0].view(np.uint32))
    np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    assert got[1] == ref[1] == want_one[1] and got[1].blocks == 50 * SPF // 2400 - 3


# ---------------------------------------------------------------- api
def test_api_loudness_against_the_fixture():
    g = np.load(GOLDEN)
    for name in ("gated_noise", "speech_like"):
        got = api.loudness(make_signal(name))
        assert abs(got - float(g[name + "_lufs"])) <= TOL_LU, (name, got)
    assert abs(api.loudness(api.AudioBuffer(make_signal("sine"), 24000)) - (-3.01)) <= 0.1
    with pytest.raises(ValueError):
        api.loudness(api.AudioBuffer(np.zeros(100, np.float32), 16000))


# ---------------------------------------------------------------- CLI
def test_cli_target_lufs(tmp_path, capsys):
    """--streaming --target-lufs: the dump is the one-shot stage (normaliser, then the -1 dB ceiling the flag brings with it) on
    the plain streaming run's PCM, and the run prints the measured loudness and the final gain."""
    from qwen3_tts_rs_amd import cli
    args = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7"]
    assert cli.main(args + ["--output-dir", str(tmp_path / "o"), "--streaming"]) == 0
    pcm24 = np.fromfile(tmp_path / "o" / "audio_seed7_frames9.bin", dtype="<f4")
    capsys.readouterr()
    assert cli.main(args + ["--output-dir", str(tmp_path / "o2"), "--streaming", "--target-lufs", "-19", "--prior-gain-db", "-3"]) == 0
    out = capsys.readouterr().out
    got = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    ref, reading = one_shot(pcm24, loud=(NORM, -1900, -300), level=(0, -100))
    np.testing.assert_array_equal(got.view(np.uint32), ref.view(np.uint32))
    assert f"Loudness: {reading.lufs:.2f} LUFS" in out and f"final gain {reading.gain_db:+.2f} dB" in out
    assert cli.main(args + ["--output-dir", str(tmp_path / "o3"), "--target-lufs", "-19"]) == 2      # not without --streaming
