"""Streamed audio at a requested sample rate, f32 or PCM16, through every layer that streams: the codec stream
(q3_codec_stream_push_out), the session (q3_session_set_output / _next_chunks_out), the batcher's streamed tickets
(q3_batcher_ticket_output / _read_out) and the CLI. Everywhere the converted stream must be, bit for bit, the one-shot output stage
(api.resample_gpu) applied to the 24 kHz f32 PCM the same path delivers without conversion. Tiny synthetic model (q.tiny())."""
import ctypes
import wave

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _batcher, _drive, _cat


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def one_shot(pcm, rate, s16):
    return api.resample_gpu(pcm, rate, pcm16=s16).samples


# ---------------------------------------------------------------- codec stream
@pytest.mark.gpu
def test_codec_stream_push_out(gm):
    """40 random frames to two rows in pieces 1, 2, 9, 13, 15: row 0 at 16 kHz s16, row 1 at 48 kHz f32 (stage rows 1 and 0: the
    stage row is the caller's choice). A push without a stage on the same stream object keeps today's bits."""
    rng = np.random.default_rng(5)
    codes = {r: rng.integers(0, 2048, size=(40, 16)).astype(np.uint32) for r in (0, 1)}
    whole = {r: gm.decode_codes(codes[r]).samples.copy() for r in (0, 1)}
    fmt = {0: (16000, True), 1: (48000, False)}
    srow = {0: 1, 1: 0}
    cs = gm.codec_stream(2, 40)
    ps = gm.pcm_stage(2, 40 * SPF)
    for r in (0, 1):
        ps.set(srow[r], *fmt[r])
    got = {0: [], 1: []}; at = 0
    pieces = [1, 2, 9, 13, 15]
    for k, n in enumerate(pieces):
        out = cs.push({r: codes[r][at:at + n] for r in (0, 1)}, stage=ps, stage_rows=srow, last=(0, 1) if k == len(pieces) - 1 else ())
        at += n
        for r in (0, 1):
            got[r].append(out[r])
            assert cs.pos(r) == at
    for r in (0, 1):
        g = np.concatenate(got[r])
        assert g.dtype == (np.int16 if fmt[r][1] else np.float32)
        np.testing.assert_array_equal(g, one_shot(whole[r], *fmt[r]), err_msg=f"row {r}")
    # a flush without frames on a row that was flushed: nothing; frames for it: refused, and the stream's row does not move
    assert cs.push({0: codes[0][:0]}, stage=ps, stage_rows=srow, last=(0,))[0].size == 0
    cs.reset(0); cs.reset(1)
    with pytest.raises(_lib.Q3Error):
        cs.push({0: codes[0][:3]}, stage=ps, stage_rows=srow)
    assert cs.pos(0) == 0
    # the same stream object without a stage: decode_codes' bits
    out = cs.push({0: codes[0][:25], 1: codes[1][:7]})
    np.testing.assert_array_equal(out[0], whole[0][:25 * SPF]); np.testing.assert_array_equal(out[1], whole[1][:7 * SPF])
    out = cs.push({0: codes[0][25:], 1: codes[1][7:]})
    np.testing.assert_array_equal(out[0], whole[0][25 * SPF:]); np.testing.assert_array_equal(out[1], whole[1][7 * SPF:])
    # the stage is the caller's: a codec-stream reset does not restart a stage row (the recovery rule) — row 1 of a fresh stage
    # takes frames 0..20, the stream row is reset and pushed again from frame 0 with nothing else said to the stage
    ps.set(0, 16000, True)
    cs.reset(1)
    a = cs.push({1: codes[1][:20]}, stage=ps, stage_rows={1: 0})[1]
    cs.reset(1)
    cs.prime(1, codes[1][:20])                         # the row's state again, no samples
    b = cs.push({1: codes[1][20:]}, stage=ps, stage_rows={1: 0}, last=(1,))[1]
    np.testing.assert_array_equal(np.concatenate([a, b]), one_shot(whole[1], 16000, True))
    cs.close(); ps.close()


# ---------------------------------------------------------------- session
def _utts(limits):
    return [q.Utterance(synthetic_prompt(8 + 3 * i, i), q.Speaker.Ryan, q.Language.English, seed=100 + i, max_length=L)
            for i, L in enumerate(limits)]


def _session(gm, limits, opts, mode):
    s = gm.session(_utts(limits), opts)
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, mode))
    return s


def _rounds(s, out, max_rounds=64):
    got = [[] for _ in range(s.B)]; done_at = [None] * s.B
    for k in range(max_rounds):
        r = s.next_chunks_out() if out else s.next_chunks()
        for b, (a, d) in enumerate(r):
            if a is not None:
                assert done_at[b] is None, b               # nothing after the call that reported the row done
                got[b].append(a)
            if d and done_at[b] is None:
                done_at[b] = k
        if all(d for _, d in r):
            return got, done_at
    raise AssertionError("the session did not finish")


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [1, 0])
def test_session_next_chunks_out(gm, mode):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 16 kHz s16: every row's chunks concatenate to the one-shot stage on the
    row's next_chunks PCM from a twin session; a row's tail comes in the call that reports it done."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    s = _session(gm, limits, opts, mode); t = _session(gm, limits, opts, mode)
    s.set_output(16000, pcm16=True)
    got, done_s = _rounds(s, True); want, done_t = _rounds(t, False)
    assert done_s == done_t
    for b, L in enumerate(limits):
        pcm = np.concatenate([a.samples for a in want[b]])
        assert pcm.shape == (L * SPF,)
        assert all(a.sample_rate == 16000 and a.samples.dtype == np.int16 for a in got[b])
        g = np.concatenate([a.samples for a in got[b]])
        assert g.size == round(L * SPF * 2 / 3)
        np.testing.assert_array_equal(g, one_shot(pcm, 16000, True), err_msg=f"row {b}")
    # the setting is fixed once the first chunk has streamed — also when that chunk left through next_chunks
    for x in (s, t):
        with pytest.raises(_lib.Q3Error) as e:
            x.set_output(8000)
        assert e.value.status == Q3_INVALID_ARG
    s.close(); t.close()


@pytest.mark.gpu
def test_session_24k_is_next_chunks(gm):
    limits = [7, 12]
    opts = q.SynthesisOptions(max_length=12, seed=42, eos_token_id=None, chunk_frames=5)
    s = _session(gm, limits, opts, 1); t = _session(gm, limits, opts, 1)
    s.set_output(24000)
    with pytest.raises(_lib.Q3Error) as e:
        s.set_output(47999)
    assert e.value.status == 7
    got, done_s = _rounds(s, True); want, done_t = _rounds(t, False)
    assert done_s == done_t
    for b in range(2):
        assert [a.samples.size for a in got[b]] == [a.samples.size for a in want[b]]
        for a, w in zip(got[b], want[b]):
            assert a.samples.dtype == np.float32
            np.testing.assert_array_equal(a.samples, w.samples)
    s.close(); t.close()


@pytest.mark.gpu
def test_session_replace_restarts_the_row(gm):
    """Row 0 ends at 6 frames and is replaced while row 1 goes on: the new utterance's stream is its own one-shot conversion."""
    opts = q.SynthesisOptions(max_length=20, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)

    def run(out):
        s = _session(gm, [6, 20], opts, 1)
        if out:
            s.set_output(8000, pcm16=True)
        parts = {"old": [], "new": [], 1: []}
        key = "old"
        for _ in range(32):
            r = s.next_chunks_out() if out else s.next_chunks()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else 1].append(a.samples)
            if r[0][1] and key == "old":
                s.replace(0, new); key = "new"
            elif all(d for _, d in r):
                break
        s.close()
        return {k: np.concatenate(v) for k, v in parts.items()}
    got, want = run(True), run(False)
    assert want["old"].size == 6 * SPF and want["new"].size == 8 * SPF and want[1].size == 20 * SPF
    for k in got:
        np.testing.assert_array_equal(got[k], one_shot(want[k], 8000, True), err_msg=str(k))


# ---------------------------------------------------------------- batcher
FIVE = [(24000, False), (8000, True), (48000, False), (16000, True), (24000, False)]


def _run_five(gm, utts, fmts):
    b = q.Batcher(gm, slots=2, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    tickets = [b.submit_streamed(u, sample_rate=sr, pcm16=s16) for u, (sr, s16) in zip(utts, fmts)]
    return b, tickets


@pytest.mark.gpu
def test_batcher_five_tickets_two_slots(gm):
    """Requests 0-4 of test_batcher_stream.py (preset voice, voice design, x-vector, ICL with 5 and with 20 reference frames;
    5 / 50 / 20 / 27 / 9 frames) through two slots: every slot changes owner, and formats, mid-run."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(5)]
    b, tickets = _run_five(gm, utts, [(24000, False)] * 5)
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    for i in range(5):
        assert want[i].shape == (LIMITS[i] * SPF,)
    b, tickets = _run_five(gm, utts, FIVE)
    # before the first step: a converted ticket is refused by the f32 read, which names the other one
    with pytest.raises(_lib.Q3Error, match="q3_batcher_read_out") as e:
        n = ctypes.c_size_t(); d = ctypes.c_int(); buf = np.zeros(16, np.float32)
        _lib.check(_lib.lib.q3_batcher_read(b._h, tickets[1], buf.ctypes.data_as(ctypes.c_void_p), 16, ctypes.byref(n), ctypes.byref(d)))
    assert e.value.status == Q3_INVALID_ARG
    plain = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_output(plain, 16000, True)               # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_output(tickets[4], 47999)
    assert e.value.status == 7
    b.step(STEP)
    for t in (tickets[0], tickets[4]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_output(t, 16000, True)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[plain] = False
    got, _ = _drive(b, tickets + [plain], streamed, cap=1000)
    for i, t in enumerate(tickets):
        sr, s16 = FIVE[i]
        g = _cat(got[t])
        assert g.dtype == (np.int16 if s16 else np.float32), i
        assert b.poll(t)[0] == q.Batcher.DONE
        np.testing.assert_array_equal(g, one_shot(want[i], sr, s16) if (sr, s16) != (24000, False) else want[i], err_msg=f"request {i}")
    # a default ticket through the C read, unchanged; read_out serves it too
    t = b.submit_streamed(utts[0])
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    half = want[0].size // 2
    a, done = b.read(t, half)
    assert not done
    buf = np.zeros(want[0].size, np.float32); n = ctypes.c_size_t(); d = ctypes.c_int()
    _lib.check(_lib.lib.q3_batcher_read_out(b._h, t, buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d)))
    assert d.value == 1
    np.testing.assert_array_equal(np.concatenate([a, buf[:n.value]]), want[0])
    b.close()


@pytest.mark.gpu
def test_batcher_cancelled_ticket_and_next_owner(gm):
    """A converted ticket cancelled mid-run delivers the conversion of the frames it committed, tail included; the slot's next
    owner starts from a fresh row."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in (1, 2)]
    b = q.Batcher(gm, slots=1, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    ref = b.run_all(utts, want_pcm=True, poll_frames=STEP)
    t0 = b.submit_streamed(utts[0], sample_rate=16000, pcm16=True); t1 = b.submit_streamed(utts[1], sample_rate=44100)
    b.step(STEP); b.step(STEP)
    b.cancel(t0)
    n0 = b.poll(t0)[1]
    assert 0 < n0 < LIMITS[1]
    got, _ = _drive(b, [t0, t1], {t0: True, t1: True})
    np.testing.assert_array_equal(_cat(got[t0]), one_shot(ref[0][1][:n0 * SPF], 16000, True))
    np.testing.assert_array_equal(_cat(got[t1]), one_shot(ref[1][1], 44100, False))
    b.close()


@pytest.mark.gpu
def test_batcher_block_limit_with_converted_tickets(gm, monkeypatch):
    """The block-limit scenario of test_batcher_stream.py (blocks of 32 frames, four at most: the joint push that needs the long
    ticket's third block is refused and repeated row by row, the long ticket alone fails) with 16 kHz s16 tickets: the
    surviving tickets' streams are the one-shot conversion of their PCM — the stage followed the delivered samples only."""
    long_i, short_i = 6, [2, 3, 10, 8, 0, 7, 4, 11, 1]
    utts = {i: _request(gm.config, i, LIMITS[i]) for i in [long_i] + short_i}
    b = _batcher(gm)
    want = dict(zip(short_i, b.run_all([utts[i] for i in short_i], want_pcm=True, poll_frames=STEP)))
    b.close()
    monkeypatch.setenv("Q3_BAT_STREAM_BLOCK_FRAMES", "32")
    monkeypatch.setenv("Q3_BAT_STREAM_MAX_BLOCKS", "4")
    b = _batcher(gm)
    tickets = [b.submit_streamed(utts[i], sample_rate=16000, pcm16=True) for i in [long_i] + short_i]
    got, _ = _drive(b, tickets[1:], {t: True for t in tickets[1:]}, step=5)
    assert b.poll(tickets[0])[0] == q.Batcher.FAILED
    with pytest.raises(_lib.Q3Error, match="block pool exhausted"):
        b.read(tickets[0], 1000)
    for i, t in zip(short_i, tickets[1:]):
        np.testing.assert_array_equal(_cat(got[t]), one_shot(want[i][1], 16000, True), err_msg=f"request {i}")
        np.testing.assert_array_equal(b.fetch(t)[0], want[i][0], err_msg=f"request {i}")
    info = b.stream_info()
    assert info["block_frames"] == 32 and info["blocks_in_use"] == 0 and info["blocks_peak"] <= 4
    b.close()


# ---------------------------------------------------------------- CLI
@pytest.mark.gpu
def test_cli_output_rate(tmp_path):
    out = tmp_path / "o"
    rc = cli.main(["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7",
                   "--output-dir", str(out), "--streaming", "--output-rate", "16000"])
    assert rc == 0
    n = 9 * SPF
    with wave.open(str(out / "audio_seed7_frames9.wav")) as w:
        assert (w.getnframes(), w.getframerate(), w.getsampwidth()) == (round(n * 2 / 3), 16000, 2)
    # the same chunks at 24 kHz, converted in one shot
    rc = cli.main(["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7",
                   "--output-dir", str(tmp_path / "o2"), "--streaming"])
    assert rc == 0
    pcm24 = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    np.testing.assert_array_equal(np.fromfile(out / "audio_seed7_frames9.bin", dtype="<f4"), one_shot(pcm24, 16000, False))
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3"), "--output-rate", "16000"]) == 2
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3"), "--streaming", "--output-rate", "47999"]) == 2
