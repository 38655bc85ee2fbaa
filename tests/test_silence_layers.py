"""The silence step through every layer that streams: the session (q3_session_set_silence / _silence /
_next_chunks_out), the batcher's streamed tickets (q3_batcher_ticket_silence / _silence_read / _read_out, parked tickets included)
and api.resample_gpu. Everywhere the stream must be, bit for bit, the one-shot stage applied to the numpy restatement
(test_silence_host.py) of the 24 kHz f32 PCM the same path delivers without the step, and the counts the restatement's. The model's
output is noise-like, so each threshold is chosen from the restatement on the row's own PCM such that something is cut. Tiny
synthetic model (q.tiny())."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt
from test_batcher_stream import LIMITS, OPTS, STEP, SPF, Q3_INVALID_ARG, _request, _drive, _cat
from test_output_format import _session
from test_silence_host import H, energies, restate

pytestmark = pytest.mark.gpu
PARKED = 5


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


def pick(pcm, edge_ms, pause_ms):
    """(threshold in mB, y, counts): the lowest of a few quantiles of the clip's own hop levels at which the step cuts something and
    keeps something"""
    e = energies(pcm).astype(np.float64) / H
    lv = 1000.0 * np.log10(np.maximum(e, 1e-12))
    for qt in (0.5, 0.7, 0.85, 0.95):
        thr = int(np.clip(round(float(np.quantile(lv, qt))), -9000, -2000))
        y, counts, _, _ = restate(pcm, thr, edge_ms, pause_ms)
        if 0 < counts[1] < counts[0]:
            return thr, y, counts
    raise AssertionError(f"no threshold cuts this clip: hop levels {lv.min():.0f} .. {lv.max():.0f} mB")


def one_shot(pcm, rate=24000, fmt="f32"):
    ps = api.PcmStage(0, 1, max(pcm.size, 1))
    try:
        ps.set(0, rate, fmt=fmt)
        return ps.push({0: pcm}, last=(0,))[0]
    finally:
        ps.close()


# ---------------------------------------------------------------- session
def test_session_silence_window_and_replace(gm):
    """B = 3, max_length 7 / 12 / 25, chunks of 3 frames, 16 kHz s16; row 0 has a setting of its own, row 1 none, row 2 another
    behind a setting for every row. Row 0 is replaced when it ends: the new utterance keeps the row's setting and starts the row
    over. Every row's chunks concatenate to the one-shot stage on the restatement of the row's next_chunks PCM from a twin session.
    After the first streamed chunk the setting is fixed."""
    limits = [7, 12, 25]
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)
    ep = {"old": (0, 20), "new": (0, 20), 2: (20, 40)}
    thr = {}
    readings = {}

    def run(kind):
        s = _session(gm, limits, opts, 1)
        if kind == "out":
            s.set_output(16000, pcm16=True)
            for bad in ((-91.0, 50, 400, 0), (-50.0, 55, 400, 0), (-50.0, 50, 10, 0), (-50.0, 50, 400, 3)):
                with pytest.raises(_lib.Q3Error) as e:
                    s.set_silence(*bad)
                assert e.value.status == Q3_INVALID_ARG
            with pytest.raises(_lib.Q3Error):
                s.silence(0)                               # no step yet: no reading
            s.set_silence(-40.0, 100, 200)                 # every row ...
            s.set_silence(thr["old"] / 100.0, *ep["old"], b=0); s.set_silence(None, b=1); s.set_silence(thr[2] / 100.0, *ep[2], b=2)      # ... and each its own
            assert tuple(s.silence(0)) == (0, 0, 0, 0, 0)  # nothing streamed yet
            with pytest.raises(_lib.Q3Error):
                s.silence(1)
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
                        s.set_silence(-50.0, 50, 400, b)
                    assert e.value.status == Q3_INVALID_ARG
            first = False
            if r[0][1] and key == "old":
                if kind == "out":
                    readings["old"] = s.silence(0)
                s.replace(0, new); key = "new"
            elif all(d for _, d in r):
                break
        if kind == "out":
            readings["new"] = s.silence(0); readings[2] = s.silence(2)
        s.close()
        return parts
    pcm = {k: _cat(v) for k, v in run("pcm").items()}
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 12 * SPF and pcm[2].size == 25 * SPF
    want = {}
    thr["old"], want["old"], c_old = pick(pcm["old"], *ep["old"])
    thr[2], want[2], c_2 = pick(pcm[2], *ep[2])
    y_new, c_new, _, _ = restate(pcm["new"], thr["old"], *ep["new"])      # the replaced row keeps the old one's setting
    got = run("out")
    for k, (y, c) in {"old": (want["old"], c_old), "new": (y_new, c_new), 2: (want[2], c_2)}.items():
        g = _cat(got[k])
        assert g.dtype == np.int16
        np.testing.assert_array_equal(g, one_shot(y, 16000, "s16"), err_msg=str(k))
        assert tuple(readings[k]) == c, (k, readings[k], c)
    np.testing.assert_array_equal(_cat(got[1]), one_shot(pcm[1], 16000, "s16"))      # the row without the step
    assert c_old[1] < c_old[0] and c_2[1] < c_2[0]


# ---------------------------------------------------------------- batcher
def _batcher(gm, slots, **kw):
    return q.Batcher(gm, slots=slots, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS), **kw)


@pytest.fixture(scope="module")
def plain(gm):
    """requests 0-3 of test_batcher_stream.py (5 / 50 / 20 / 27 frames), their 24 kHz f32 PCM as plain streamed tickets, and for
    the first three a setting (threshold mB, edge, pause) that cuts it, with the restated y and counts"""
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(4)]
    b = _batcher(gm, 2)
    tickets = [b.submit_streamed(u) for u in utts]
    want, _ = _drive(b, tickets, {t: True for t in tickets})
    want = [_cat(want[t]) for t in tickets]
    b.close()
    cut = []
    for w, (e, p) in zip(want, ((0, 20), (20, 40), (0, 30))):      # (request 3 stays plain: no hop of its PCM is under -20 dBFS)
        t, y, c = pick(w, e, p)
        cut.append(((t, e, p), y, c))
    for w in want:
        w.setflags(write=False)
    return utts, want, cut


def _sil(setting):
    return (setting[0] / 100.0, setting[1], setting[2])


def test_batcher_tickets_with_their_own_setting(gm, plain):
    """Two slots: a trimmed ticket at 8 kHz mu-law beside a plain one; then, in the slots they leave, another setting at 24 kHz f32
    (read through read_out, in pieces) and a ticket without the step in a row that had it. The counts are final once `read` has
    reported the ticket done and stay until `fetch`."""
    utts, want, cut = plain
    four = [dict(sample_rate=8000, fmt="ulaw", silence=_sil(cut[0][0])), dict(), dict(silence=_sil(cut[2][0])), dict(sample_rate=16000, fmt="s16")]
    b = _batcher(gm, 2)
    tickets = [b.submit_streamed(u, **kw) for u, kw in zip(utts, four)]
    closed = b.submit(utts[0], want_pcm=False)
    with pytest.raises(_lib.Q3Error):
        b.ticket_silence(closed, -50.0, 50, 400)           # not a streamed ticket
    with pytest.raises(_lib.Q3Error) as e:
        b.ticket_silence(tickets[3], -50.0, 50, 2010)
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error):
        b.silence(tickets[1])                              # a ticket without the step has no reading
    assert tuple(b.silence(tickets[2])) == (0, 0, 0, 0, 0)
    b.step(STEP)
    for t in (tickets[0], tickets[3]):                     # running, and still queued: both have been through a step
        with pytest.raises(_lib.Q3Error) as e:
            b.ticket_silence(t, -50.0, 50, 400)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[closed] = False
    got, _ = _drive(b, tickets + [closed], streamed, cap=1000)
    refs = [one_shot(cut[0][1], 8000, "ulaw"), want[1], cut[2][1], one_shot(want[3], 16000, "s16")]
    for i, t in enumerate(tickets):
        assert b.poll(t)[0] == q.Batcher.DONE
        g = _cat(got[t])
        assert g.dtype == refs[i].dtype
        np.testing.assert_array_equal(g.view(np.uint8), refs[i].view(np.uint8), err_msg=f"request {i}")
        if i in (0, 2):
            assert tuple(b.silence(t)) == cut[i][2], i      # final after `done`
            assert sum(x.size for x in got[t]) == refs[i].size      # read_out's counts: what the step handed on
    b.fetch(tickets[0])
    with pytest.raises(_lib.Q3Error):
        b.silence(tickets[0])                              # released
    b.close()


def test_a_slots_next_owner_starts_from_its_own_setting(gm, plain):
    """One slot: a trimmed ticket, then one without the step in the row that had it, then another setting."""
    utts, want, cut = plain
    b = _batcher(gm, 1)
    A = b.submit_streamed(utts[1], silence=_sil(cut[1][0]))
    B = b.submit_streamed(utts[2])
    C = b.submit_streamed(utts[0], silence=_sil(cut[0][0]))
    got, _ = _drive(b, [A, B, C], {A: True, B: True, C: True})
    for t, ref, c in ((A, cut[1][1], cut[1][2]), (B, want[2], None), (C, cut[0][1], cut[0][2])):
        np.testing.assert_array_equal(_cat(got[t]).view(np.uint32), ref.view(np.uint32))
        if c is not None:
            assert tuple(b.silence(t)) == c
    b.close()


def test_a_parked_and_resumed_ticket_equals_the_uninterrupted_one(gm, plain):
    """The ticket is parked in slot 0 and goes on in slot 1: its stage row follows it, the step's state included."""
    utts, want, cut = plain

    def run(park):
        b = _batcher(gm, 2, **(dict(max_parked=2) if park else {}))
        S = b.submit_streamed(utts[1], silence=_sil(cut[1][0]))            # 50 frames
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
        r = b.silence(S)
        if park:
            assert b.park_info()["moved"] == 1
        b.close()
        return _cat([x for x in got if x.size]), r

    ref, got = run(False), run(True)
    np.testing.assert_array_equal(ref[0].view(np.uint32), cut[1][1].view(np.uint32))
    np.testing.assert_array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    assert tuple(got[1]) == tuple(ref[1]) == cut[1][2]


# ---------------------------------------------------------------- api
def test_resample_gpu_against_trim_silence(plain):
    utts, want, cut = plain
    (thr, e, p), y, c = cut[1]
    x = want[1]
    host, counts = api.trim_silence(x, thr / 100.0, e, p, counts=True)
    assert tuple(counts) == c and (host.view(np.uint32) == y.view(np.uint32)).all()
    dev = api.resample_gpu(x, 24000, silence=(thr / 100.0, e, p))
    np.testing.assert_array_equal(dev.samples.view(np.uint32), host.view(np.uint32))
    dev16 = api.resample_gpu(api.AudioBuffer(x, 24000), 16000, pcm16=True, tempo_permille=1250, silence=(thr / 100.0, e, p))
    np.testing.assert_array_equal(dev16.samples, api.resample_gpu(host, 16000, pcm16=True, tempo_permille=1250).samples)
    assert isinstance(api.trim_silence(api.AudioBuffer(x, 24000), thr / 100.0, e, p), api.AudioBuffer)
    with pytest.raises(ValueError):
        api.trim_silence(api.AudioBuffer(x, 16000), -50.0)
