"""G.711 output and a level per row through every layer that streams: the codec stream (q3_codec_stream_push_out
through a stage row), the session (q3_session_set_output / _set_level / _next_chunks_out), the batcher's streamed tickets
(q3_batcher_ticket_output / _ticket_level / _read_out) and the CLI. Everywhere the stream must be, byte for byte, the one-shot
stage (api.resample_gpu with fmt= and gain_mb= / ceiling_mb=) applied to the 24 kHz f32 PCM the same path delivers without it.
Tiny synthetic model (q.tiny())."""
import ctypes
import struct

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api, cli
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session
from test_g711 import parse_wav

LEVEL = (600, -100)


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def one_shot(pcm, rate, fmt, level=(0, 0)):
    return api.resample_gpu(pcm, rate, fmt=fmt, gain_mb=level[0], ceiling_mb=level[1]).samples


# ---------------------------------------------------------------- codec stream
@pytest.mark.gpu
def test_codec_stream_push_out_ulaw_with_level(gm):
    """40 random frames to two rows in pieces 1, 2, 9, 13, 15: row 0 at 8 kHz ulaw with a level, row 1 at 24 kHz alaw without."""
    rng = np.random.default_rng(5)
    codes = {r: rng.integers(0, 2048, size=(40, 16)).astype(np.uint32) for r in (0, 1)}
    whole = {r: gm.decode_codes(codes[r]).samples.copy() for r in (0, 1)}
    fmt = {0: (8000, "ulaw", LEVEL), 1: (24000, "alaw", (0, 0))}
    ps = gm.pcm_stage(2, 40 * SPF)
    cs = gm.codec_stream(2, 40)
    for r, (sr, f, lv) in fmt.items():
        ps.set(r, sr, fmt=f); ps.set_level(r, *lv)
    got = {0: [], 1: []}; at = 0
    pieces = [1, 2, 9, 13, 15]
    for k, n in enumerate(pieces):
        out = cs.push({r: codes[r][at:at + n] for r in (0, 1)}, stage=ps, last=(0, 1) if k == len(pieces) - 1 else ())
        at += n
        for r in (0, 1):
            got[r].append(out[r])
    cs.close(); ps.close()
    for r, (sr, f, lv) in fmt.items():
        g = np.concatenate(got[r])
        assert g.dtype == np.uint8
        np.testing.assert_array_equal(g, one_shot(whole[r], sr, f, lv), err_msg=f"row {r}")
    assert np.concatenate(got[0]).size == 40 * SPF // 3 and np.concatenate(got[1]).size == 40 * SPF


# ---------------------------------------------------------------- session
@pytest.mark.gpu
def test_session_ulaw_and_level(gm):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 8 kHz ulaw; levels (+600, -100) / off / (+1200, -300); row 0 is replaced
    when it ends: the new utterance keeps the row's level and starts the row over. Every row's chunks concatenate to the one-shot
    stage on the row's next_chunks PCM from a twin session."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)

    def run(kind):
        s = _session(gm, limits, opts, 1)
        if kind == "out":
            s.set_output(8000, fmt="ulaw")
            with pytest.raises(_lib.Q3Error) as e:
                s.set_level(2401, -100, 0)
            assert e.value.status == Q3_INVALID_ARG
            with pytest.raises(_lib.Q3Error):
                s.set_level(600, -100, 3)                  # no such row
            s.set_level(300, -50)                          # every row ...
            s.set_level(*LEVEL, 0); s.set_level(0, 0, 1); s.set_level(1200, -300, 2)      # ... and each its own
        parts = {"old": [], "new": [], 1: [], 2: []}
        key = "old"; first = True
        for _ in range(32):
            r = s.next_chunks() if kind == "pcm" else s.next_chunks_out()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else b].append(a.samples)
            if first and kind == "out":
                for b in (0, 2, -1):                       # every row has delivered its first chunk: the setting is fixed
                    with pytest.raises(_lib.Q3Error) as e:
                        s.set_level(100, -100, b)
                    assert e.value.status == Q3_INVALID_ARG
            first = False
            if r[0][1] and key == "old":
                s.replace(0, new); key = "new"
            elif all(d for _, d in r):
                break
        s.close()
        return parts
    got, want = run("out"), run("pcm")
    pcm = {k: np.concatenate(v) for k, v in want.items()}
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 12 * SPF and pcm[2].size == 25 * SPF
    level = {"old": LEVEL, "new": LEVEL, 1: (0, 0), 2: (1200, -300)}
    for k, lv in level.items():
        g = np.concatenate(got[k])
        assert g.dtype == np.uint8 and g.size == pcm[k].size // 3, k
        np.testing.assert_array_equal(g, one_shot(pcm[k], 8000, "ulaw", lv), err_msg=str(k))


# ---------------------------------------------------------------- batcher
@pytest.mark.gpu
def test_batcher_tickets_ulaw_and_level(gm):
    """Requests 0-3 of test_batcher_stream.py (5 / 50 / 20 / 27 frames) through two slots: 8 kHz ulaw with a level beside a plain
    ticket; then, in the slots they leave, a level at 24 kHz f32 (read through read_out) and 8 kHz alaw without a level in a
    row that had one."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(4)]
    four = [(8000, "ulaw", LEVEL), (24000, "f32", (0, 0)), (24000, "f32", (1200, -100)), (8000, "alaw", (0, 0))]

    def batcher():
        return q.Batcher(gm, slots=2, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    b = batcher()
    tickets = [b.submit_streamed(u) for u in utts]
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    b = batcher()
    tickets = [b.submit_streamed(u, sample_rate=sr, fmt=f, gain_mb=lv[0], ceiling_mb=lv[1]) for u, (sr, f, lv) in zip(utts, four)]
    plain = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_level(plain, 600, -100)                   # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_level(tickets[3], 600, 1)
    assert e.value.status == Q3_INVALID_ARG
    b.step(STEP)
    for t in (tickets[0], tickets[3]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_level(t, 100, -100)
        assert e.value.status == Q3_INVALID_ARG
    # q3_batcher_read refuses a ticket with a byte format and names the call that serves it
    buf = np.zeros(16, np.float32); n = ctypes.c_size_t(); d = ctypes.c_int()
    st = _lib.lib.q3_batcher_read(b._h, tickets[0], buf.ctypes.data_as(ctypes.c_void_p), buf.size, ctypes.byref(n), ctypes.byref(d))
    assert st == Q3_INVALID_ARG and b"q3_batcher_read_out" in _lib.lib.q3_last_error() and b"ulaw" in _lib.lib.q3_last_error()
    streamed = {t: True for t in tickets}; streamed[plain] = False
    got, _ = _drive(b, tickets + [plain], streamed, cap=1000)
    for i, t in enumerate(tickets):
        sr, f, lv = four[i]
        g = _cat(got[t])
        assert g.dtype == api.PCM_DTYPE[api.PCM_NAMES.index(f)], i
        assert b.poll(t)[0] == q.Batcher.DONE
        np.testing.assert_array_equal(g, one_shot(want[i], sr, f, lv) if (sr, f, lv) != (24000, "f32", (0, 0)) else want[i], err_msg=f"request {i}")
    b.close()


@pytest.mark.gpu
def test_cancelled_tickets_slot_gives_its_next_owner_its_own_setting(gm):
    """One slot. A ticket at 8 kHz ulaw with a level is cancelled in mid-run; the next owner of its slot (16 kHz s16, no level)
    and the one after (8 kHz alaw, another level) each get their own output."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in (1, 2, 3)]

    def batcher():
        return q.Batcher(gm, slots=1, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    b = batcher()
    tickets = [b.submit_streamed(u) for u in utts]
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    b = batcher()
    A = b.submit_streamed(utts[0], sample_rate=8000, fmt="ulaw", gain_mb=LEVEL[0], ceiling_mb=LEVEL[1])
    B = b.submit_streamed(utts[1], sample_rate=16000, fmt="s16")
    C = b.submit_streamed(utts[2], sample_rate=8000, fmt="alaw", gain_mb=1200, ceiling_mb=-300)
    b.step(STEP); b.step(STEP)
    assert b.poll(A)[0] == q.Batcher.RUNNING
    b.cancel(A)
    got, _ = _drive(b, [A, B, C], {A: True, B: True, C: True})
    a = _cat(got[A])
    assert a.dtype == np.uint8 and 0 < a.size < LIMITS[1] * SPF // 3
    # the frames A committed, flushed: the one-shot stage on that much of its PCM
    n24 = b.poll(A)[1] * SPF
    np.testing.assert_array_equal(a, one_shot(want[0][:n24], 8000, "ulaw", LEVEL))
    np.testing.assert_array_equal(_cat(got[B]), one_shot(want[1], 16000, "s16"))
    np.testing.assert_array_equal(_cat(got[C]), one_shot(want[2], 8000, "alaw", (1200, -300)))
    b.close()


# ---------------------------------------------------------------- CLI
@pytest.mark.gpu
def test_cli_ulaw(tmp_path):
    out = tmp_path / "o"
    args = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "9", "--no-eos", "--seed", "7"]
    rc = cli.main(args + ["--output-dir", str(out), "--streaming", "--output-rate", "8000", "--output-format", "ulaw", "--gain-db", "6",
                          "--ceiling-db", "-1"])
    assert rc == 0
    w = parse_wav(str(out / "audio_seed7_frames9.wav"))
    assert w["fmt"] == (7, 1, 8000, 8000, 1, 8, 0) and w["fact"] == 9 * SPF // 3 and len(w["data"]) == 9 * SPF // 3
    rc = cli.main(args + ["--output-dir", str(tmp_path / "o2"), "--streaming"])
    assert rc == 0
    pcm24 = np.fromfile(tmp_path / "o2" / "audio_seed7_frames9.bin", dtype="<f4")
    np.testing.assert_array_equal(np.frombuffer(w["data"], np.uint8), one_shot(pcm24, 8000, "ulaw", (600, -100)))
    rc = cli.main(args + ["--output-dir", str(tmp_path / "o4"), "--streaming", "--output-rate", "8000", "--output-format", "alaw"])
    assert rc == 0 and parse_wav(str(tmp_path / "o4" / "audio_seed7_frames9.wav"))["fmt"][0] == 6
    for extra in (["--output-format", "ulaw"], ["--gain-db", "6"], ["--ceiling-db", "-1"]):      # not without --streaming
        assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3")] + extra) == 2
    assert cli.main(["--synthetic", "tiny", "--frames", "9", "--output-dir", str(tmp_path / "o3"), "--streaming", "--gain-db", "30"]) == 2
