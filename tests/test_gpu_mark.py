"""The keyed watermark on the GPU: k_mark in the output stage against q3_mark_embed bit for bit however the stream is
cut into pushes and rows, the commit rule, the chain around it, the device detector (k_mark_fold, k_mark_corr) against the float64
host detector, the round trip through the stage's own formats and the intake, and the session, batcher and CLI layers. Tiny
synthetic model (q.tiny()) where a model is needed. Measured figures are printed before they are asserted."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
import mark_cases as M
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session

pytestmark = pytest.mark.gpu
T = api.MARK_SCORE_DETECT
KEY = 0xC0FFEE


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


@pytest.fixture(scope="module")
def sig():
    """10 007 samples (more than two periods of the carrier, no multiple of the hop) with a stretch of digital silence, a NaN and an
    inf, and its host-marked twins"""
    x = M.speechlike(3, 0.5)[:10007].copy()
    x[3000:4500] = 0.0
    x[5001] = np.nan; x[7003] = np.inf
    x.setflags(write=False)
    return x


def stream(x, cut, key=KEY, db=-26.0, rate=24000, fmt="f32"):
    ps = api.PcmStage(0, 1, max(cut, 1))
    try:
        ps.set(0, rate, fmt=fmt)
        if key:
            ps.set_mark(0, key, db)
        out = [ps.push({0: x[i:i + cut]}, last=(0,) if i + cut >= x.size else ())[0] for i in range(0, x.size, cut)]
        return np.concatenate(out)
    finally:
        ps.close()


# ---------------------------------------------------------------- the stage
@pytest.mark.parametrize("cut", [10007, 1, 239, 240, 241, 1920, 5000])
def test_stage_is_the_host_function_however_the_stream_is_cut(sig, cut):
    want = M.lib_embed(sig, KEY, -2600)
    got = stream(sig, cut)
    assert got.dtype == np.float32 and got.size == sig.size
    np.testing.assert_array_equal(bits(got), bits(want))


def test_three_rows_with_their_own_settings_and_one_without(sig):
    """rows 0..2: their own key, strength and push size, in the same pushes; row 3 has the step off and another output: its bits are
    those of a stage on which no row was ever marked"""
    sets = [(KEY, -20.0, 700), (0x1234, -33.5, 1919), (2 ** 64 - 1, -10.0, 4100)]
    xs = [sig, sig[::-1].copy(), np.roll(sig, 1234)]
    plain_cut = 1000
    ps = api.PcmStage(0, 4, 5000)
    ref = api.PcmStage(0, 1, 5000)
    try:
        for r, (k, db, _) in enumerate(sets):
            ps.set_mark(r, k, db)
        ps.set(3, 16000, fmt="s16"); ref.set(0, 16000, fmt="s16")
        cuts = [c for _, _, c in sets] + [plain_cut]
        pos = [0] * 4
        got = [[] for _ in range(4)]
        want3 = []
        data = xs + [sig]
        while any(p < sig.size for p in pos):
            push = {r: data[r][pos[r]:pos[r] + cuts[r]] for r in range(4) if pos[r] < sig.size}
            last = tuple(r for r in push if pos[r] + cuts[r] >= sig.size)
            out = ps.push(push, last=last)
            if 3 in push:
                want3.append(ref.push({0: push[3]}, last=(0,) if 3 in last else ())[0])
            for r in push:
                got[r].append(out[r]); pos[r] += cuts[r]
        for r, (k, db, c) in enumerate(sets):
            np.testing.assert_array_equal(bits(np.concatenate(got[r])), bits(stream(xs[r], c, k, db)), err_msg=f"row {r}")
            np.testing.assert_array_equal(bits(np.concatenate(got[r])), bits(M.lib_embed(xs[r], k, api.mark_mb(db))), err_msg=f"row {r}")
        np.testing.assert_array_equal(np.concatenate(got[3]), np.concatenate(want3))
        assert np.concatenate(got[3]).dtype == np.int16
    finally:
        ps.close(); ref.close()


def test_step_off_passes_the_samples_and_is_kept_by_the_other_setters(sig):
    np.testing.assert_array_equal(bits(stream(sig, 1920, key=0)), bits(sig))           # off: 24 kHz f32 leaves as it came
    want = M.lib_embed(sig, KEY, -2500)
    ps = api.PcmStage(0, 2, sig.size)
    try:
        ps.set_mark(1, KEY, -25.0)
        ps.set(1, 24000); ps.set_tempo(1, 1000); ps.set_level(1, 0, 0); ps.reset(1)      # every one of them keeps the mark
        np.testing.assert_array_equal(bits(ps.push({1: sig}, last=(1,))[1]), bits(want))
        ps.set_mark(1, 0x77, -25.0)                                                      # another key: the row's table is rebuilt
        np.testing.assert_array_equal(bits(ps.push({1: sig}, last=(1,))[1]), bits(M.lib_embed(sig, 0x77, -2500)))
        ps.set_mark(1, None)                                                             # off again
        np.testing.assert_array_equal(bits(ps.push({1: sig}, last=(1,))[1]), bits(sig))
        for bad in (-40.01, -9.99):
            with pytest.raises(_lib.Q3Error) as e:
                ps.set_mark(0, KEY, bad)
            assert e.value.status == Q3_INVALID_ARG and "q3_pcm_stage_set_mark: strength" in str(e.value) and "out of range (-4000..-1000)" in str(e.value)
        with pytest.raises(_lib.Q3Error):
            ps.set_mark(2, KEY)
    finally:
        ps.close()


def test_a_refused_push_leaves_the_row_where_it_was(sig):
    want = M.lib_embed(sig, KEY, -2600)
    ps = api.PcmStage(0, 1, 4000)
    try:
        ps.set_mark(0, KEY)
        a = ps.push({0: sig[:3100]})[0]
        with pytest.raises(_lib.Q3Error) as e:
            ps._push_lists([0], [sig[3100:6100]], [False], cap=[2999])                 # a cap too small
        assert e.value.status == Q3_INVALID_ARG
        with pytest.raises(_lib.Q3Error):
            ps._push_lists([0], [sig[3100:7200]], [False])                             # more than the stage takes per push
        b = ps.push({0: sig[3100:6100]})[0]
        c = ps.push({0: sig[6100:]}, last=(0,))[0]
        np.testing.assert_array_equal(bits(np.concatenate([a, b, c])), bits(want))
    finally:
        ps.close()


def test_chain_order_with_tempo_loudness_and_level():
    """tempo and loudness in front of the mark, the level behind it: the stream is level(mark(loudness(tempo(x)))) with the host
    function in the mark's place and one-shot stages for its neighbours, and the ceiling holds behind the mark"""
    x = M.speechlike(8, 2.0)
    ceil_mb = -300
    front = api.resample_gpu(x, 24000, tempo_permille=1250, target_mb=-1600, prior_mb=600).samples
    marked = M.lib_embed(front, KEY, -1000)
    want = api.resample_gpu(marked, 16000, pcm16=True, gain_mb=300, ceiling_mb=ceil_mb).samples
    ps = api.PcmStage(0, 1, 9000)
    try:
        ps.set(0, 16000, pcm16=True); ps.set_tempo(0, 1250); ps.set_loudness(0, api.LOUD_NORMALIZE, -1600, 600)
        ps.set_level(0, 300, ceil_mb); ps.set_mark(0, KEY, -10.0)
        got = np.concatenate([ps.push({0: x[i:i + 9000]}, last=(0,) if i + 9000 >= x.size else ())[0] for i in range(0, x.size, 9000)])
    finally:
        ps.close()
    np.testing.assert_array_equal(got, want)
    f = api.resample_gpu(x, 24000, tempo_permille=1250, target_mb=-1600, prior_mb=600, gain_mb=300, ceiling_mb=ceil_mb, mark=(KEY, -10.0)).samples
    c = np.float32(10.0 ** (ceil_mb / 2000.0))
    unmarked = api.resample_gpu(front, 24000, gain_mb=300, ceiling_mb=ceil_mb).samples
    print(f"peak behind the level step {np.abs(f).max():.6f}, ceiling {c:.6f}; samples the mark moved: {(f != unmarked).mean():.3f}")
    assert np.abs(f).max() <= c and (f != unmarked).mean() > 0.5


# ---------------------------------------------------------------- the detector on the device
@pytest.fixture(scope="module")
def six():
    """6 s clips at 24 kHz with their float64 host readings: marked, marked and cut from the front, unmarked, another key's mark"""
    x = M.speechlike(21, 6.0)
    y = M.lib_embed(x, KEY)
    z = y.copy(); z[9000:9100] = np.nan; z[50000:56000] = 0.0
    cases = {"marked": y, "cut 12345": y[12345:], "cut 1": y[1:], "unmarked": x, "other key": M.lib_embed(x, 0xBEEF), "holes": z}
    return {k: (np.ascontiguousarray(v), M.lib_detect(v, KEY)) for k, v in cases.items()}


@pytest.mark.parametrize("name", ["marked", "cut 12345", "cut 1", "unmarked", "other key", "holes"])
def test_device_detector_against_the_f64_host_detector(six, name):
    clip, (score, offset) = six[name]
    ref = api.RefAudio.from_samples(clip, 24000, "f32")
    try:
        r = ref.mark_score(KEY)
    finally:
        ref.close()
    print(f"{name}: device score {r.score:.6f} offset {r.offset}, host f64 {score:.6f} offset {offset}, relative {abs(r.score - score) / score:.2e}")
    assert abs(r.score - score) <= 1e-3 * abs(score)
    assert r.offset == offset
    assert r.detected == (score >= T)


def test_device_detector_refusals():
    ref = api.RefAudio.from_samples(np.zeros(2 * M.P - 1, np.float32), 24000, "f32")
    try:
        with pytest.raises(_lib.Q3Error) as e:
            ref.mark_score(KEY)
        assert e.value.status == Q3_INVALID_ARG and "at least 8192" in str(e.value)
    finally:
        ref.close()
    ref = api.RefAudio.from_samples(np.zeros(2 * M.P, np.float32), 24000, "f32")
    try:
        with pytest.raises(_lib.Q3Error):
            ref.mark_score(0)
        assert ref.mark_score(KEY).score == 0.0                                        # digital silence scores nothing
    finally:
        ref.close()


@pytest.mark.parametrize("rate, fmt", [(16000, "s16"), (8000, "ulaw")])
def test_round_trip_through_the_stage_and_the_intake(rate, fmt):
    """A clip marked by the stage leaves at `rate` in `fmt`, comes back through the intake in that format and is scored on the
    device. The CPU run of the same round trip (q3_resample + the host G.711 helpers, tools/dev/mark_ab.py --threshold,
    profiles/mark_ab.txt) kept every marked 6 s clip above 1.5 x the threshold and every null clip under threshold / 1.5 in both
    formats, so the same margins are asserted here."""
    x = M.speechlike(22, 6.0)
    out = api.resample_gpu(x, rate, fmt=fmt, mark=KEY).samples
    null = api.resample_gpu(x, rate, fmt=fmt).samples
    scores = []
    for clip in (out, null):
        ref = api.RefAudio.from_samples(clip, rate, fmt)
        try:
            scores.append(ref.mark_score(KEY))
        finally:
            ref.close()
    host = M.lib_detect(M.host_round_trip(M.lib_embed(x, KEY), rate, fmt), KEY)
    print(f"round trip {rate} Hz {fmt}: device marked {scores[0].score:.3f} offset {scores[0].offset}, device null {scores[1].score:.3f}; "
          f"host round trip marked {host[0]:.3f} offset {host[1]}; threshold {T}")
    assert scores[0].score >= 1.5 * T and scores[0].detected
    assert scores[1].score <= T / 1.5 and not scores[1].detected
    assert scores[0].offset == host[1] == 0


# ---------------------------------------------------------------- session and batcher
@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def test_session_rows_with_their_own_mark_and_the_window(gm):
    """B = 3, chunks of 3 frames: rows 0 and 2 marked with their own key and strength, row 1 not. Every row's chunks concatenate to
    the host function on the row's next_chunks PCM from a twin session (row 1: to that PCM). After the first streamed chunk the
    setter is refused and changes no row."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    marks = {0: (KEY, -20.0), 2: (0x5EED, -14.0)}

    def run(out):
        s = _session(gm, limits, opts, 1)
        if out:
            with pytest.raises(_lib.Q3Error) as e:
                s.set_mark(KEY, -5.0)
            assert e.value.status == Q3_INVALID_ARG and "q3_session_set_mark: strength -500 mB out of range (-4000..-1000)" in str(e.value)
            with pytest.raises(_lib.Q3Error):
                s.set_mark(KEY, b=3)
            s.set_mark(0xAAAA, -30.0)                                                  # every row ...
            for b, (k, db) in marks.items():
                s.set_mark(k, db, b=b)                                                 # ... and each its own
            s.set_mark(None, b=1)
        parts = [[] for _ in limits]
        first = True
        for _ in range(32):
            r = s.next_chunks_out() if out else s.next_chunks()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[b].append(a.samples)
            if first and out:
                for b in (0, 1, -1):
                    with pytest.raises(_lib.Q3Error) as e:
                        s.set_mark(0xBAD, -20.0, b=b)
                    assert e.value.status == Q3_INVALID_ARG and "has streamed its first chunk: the mark is set before it" in str(e.value)
            first = False
            if all(d for _, d in r):
                break
        s.close()
        return [_cat(p) for p in parts]
    pcm = run(False)
    got = run(True)
    for b, L in enumerate(limits):
        assert pcm[b].size == L * SPF
        want = M.lib_embed(pcm[b], marks[b][0], api.mark_mb(marks[b][1])) if b in marks else pcm[b]
        np.testing.assert_array_equal(bits(got[b]), bits(want), err_msg=f"row {b}")
        if b in marks:
            assert M.lib_detect(got[b], marks[b][0])[0] > M.lib_detect(pcm[b], marks[b][0])[0]


def test_batcher_ticket_with_a_mark_and_the_slots_next_owner(gm):
    """One slot: a marked ticket, then one with no mark in the row that had it (bit-equal to a plain run), then another key at
    16 kHz s16. The setter's window closes with the first step."""
    utts = [_request(gm.config, i, LIMITS[i]) for i in (2, 0, 3)]

    def batcher():
        return q.Batcher(gm, slots=1, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS))
    b = batcher()
    tickets = [b.submit_streamed(u) for u in utts]
    plain, _ = _drive(b, tickets, {t: True for t in tickets})
    plain = [_cat(plain[t]) for t in tickets]
    b.close()
    b = batcher()
    A = b.submit_streamed(utts[0], mark=(KEY, -20.0))
    B = b.submit_streamed(utts[1])
    C = b.submit_streamed(utts[2], sample_rate=16000, pcm16=True, mark=0x77)
    closed = b.submit(utts[1], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_mark(closed, KEY)                                                     # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_mark(B, KEY, -41.0)
    assert e.value.status == Q3_INVALID_ARG and "q3_batcher_ticket_mark: strength -4100 mB" in str(e.value)
    b.step(1)
    for t in (A, B):                                                                   # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_mark(t, KEY)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {A: True, B: True, C: True, closed: False}
    got, _ = _drive(b, [A, B, C, closed], streamed)
    b.close()
    np.testing.assert_array_equal(bits(_cat(got[A])), bits(M.lib_embed(plain[0], KEY, -2000)))
    np.testing.assert_array_equal(bits(_cat(got[B])), bits(plain[1]))
    want_c = api.resample_gpu(M.lib_embed(plain[2], 0x77, -2600), 16000, pcm16=True).samples
    g = _cat(got[C])
    assert g.dtype == np.int16
    np.testing.assert_array_equal(g, want_c)


# ---------------------------------------------------------------- CLI
def test_cli_marks_a_streamed_run_and_detects_it(tmp_path, capsys):
    from qwen3_tts_rs_amd import cli
    args = ["--synthetic", "tiny", "--text", "The quick brown fox", "--frames", "50", "--no-eos", "--seed", "7", "--streaming"]
    assert cli.main(args + ["--output-dir", str(tmp_path / "p")]) == 0
    assert cli.main(args + ["--output-dir", str(tmp_path / "o"), "--watermark-key", "c0ffee"]) == 0
    assert "Watermark: key c0ffee at -26.0 dB" in capsys.readouterr().out
    plain = np.fromfile(tmp_path / "p" / "audio_seed7_frames50.bin", dtype="<f4")
    got = np.fromfile(tmp_path / "o" / "audio_seed7_frames50.bin", dtype="<f4")
    np.testing.assert_array_equal(bits(got), bits(M.lib_embed(plain, KEY, -2600)))
    wav = str(tmp_path / "o" / "audio_seed7_frames50.wav")
    for intake in ("device", "host"):
        assert cli.main(["--detect-watermark", "c0ffee", wav, "--ref-intake", intake]) == 0
        out = capsys.readouterr().out
        print(out.strip())
        assert ": DETECTED" in out and "offset 0," in out
        assert cli.main(["--detect-watermark", "c0ffef", wav, "--ref-intake", intake]) == 0
        out = capsys.readouterr().out
        print(out.strip())
        assert "not detected" in out
