"""A row's output settings (Settings) are one value through the stage, the session and the batcher: every layer refuses
a bad value in the stage's own sentence, the whole chain of six steps runs through each layer at once, and a stage row that is
reused does not remember the order in which it was set. Tiny synthetic model (q.tiny())."""

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt
from test_batcher_stream import LIMITS, Q3_INVALID_ARG, SPF, _cat, _drive, _request
from test_output_format import _session
from test_silence_host import push_sizes
from test_silence_layers import _batcher, pick
from test_stage_chain import X

pytestmark = pytest.mark.gpu
Q3_UNSUPPORTED = 7
L = _lib.lib


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


# ---------------------------------------------------------------- 1. one sentence per refusal
# (setter, arguments that break one rule, status, [setter, arguments] accepted first, the device-free entry that shares the rule)
# One row per end of every range. The status is Q3_INVALID_ARG everywhere but at the rate, whose refusal is Q3_UNSUPPORTED in every
# layer (test_pcm_stage.py pins it for the stage).
SIL = (-5000, 50, 400)
REFUSALS = [
    ("tempo", (499,), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_pitch_plan(499, 0, None, None)),
    ("tempo", (2001,), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_pitch_plan(2001, 0, None, None)),
    ("pitch", (-1201,), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_pitch_plan(1000, -1201, None, None)),
    ("pitch", (1201,), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_pitch_plan(1000, 1201, None, None)),
    ("pitch", (1200,), Q3_INVALID_ARG, ("tempo", (800,)), lambda: L.q3_pcm_stage_pitch_plan(800, 1200, None, None)),
    ("level", (-6001, 0), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_level_coeffs(-6001, 0, None, None)),
    ("level", (2401, 0), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_level_coeffs(2401, 0, None, None)),
    ("level", (0, -2401), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_level_coeffs(0, -2401, None, None)),
    ("level", (0, 1), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_level_coeffs(0, 1, None, None)),
    ("loudness", (3, -1900, 0), Q3_INVALID_ARG, None, None),
    ("loudness", (1, -4001, 0), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_loudness_consts(-4001, 0, None, None, None, None, None)),
    ("loudness", (1, -499, 0), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_loudness_consts(-499, 0, None, None, None, None, None)),
    ("loudness", (1, -1900, -6001), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_loudness_consts(-1900, -6001, None, None, None, None, None)),
    ("loudness", (1, -1900, 2401), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_loudness_consts(-1900, 2401, None, None, None, None, None)),
    ("silence", (-9001,) + SIL[1:], Q3_INVALID_ARG, None, None),
    ("silence", (-1999,) + SIL[1:], Q3_INVALID_ARG, None, None),
    ("silence", (SIL[0], 55, SIL[2]), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(55, SIL[2], None)),
    ("silence", (SIL[0], -10, SIL[2]), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(-10, SIL[2], None)),
    ("silence", (SIL[0], 1010, SIL[2]), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(1010, SIL[2], None)),
    ("silence", (SIL[0], SIL[1], 405), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(SIL[1], 405, None)),
    ("silence", (SIL[0], SIL[1], 10), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(SIL[1], 10, None)),
    ("silence", (SIL[0], SIL[1], 2010), Q3_INVALID_ARG, None, lambda: L.q3_pcm_stage_silence_hold(SIL[1], 2010, None)),
    ("output", (24000, 4), Q3_INVALID_ARG, None, None),
    ("output", (47999, 0), Q3_UNSUPPORTED, None, lambda: L.q3_pcm_stage_taps(47999, None, 0, None, None)),
]
STAGE_FN = dict(output="q3_pcm_stage_set", tempo="q3_pcm_stage_set_tempo", pitch="q3_pcm_stage_set_pitch", level="q3_pcm_stage_set_level",
                loudness="q3_pcm_stage_set_loudness", silence="q3_pcm_stage_set_silence")


def refusal(call):
    """(status, the entry point the message names, the sentence behind it)"""
    st = call()
    who, _, text = L.q3_last_error().decode().partition(": ")
    return st, who, text


def test_every_layer_refuses_in_the_stages_words(gm):
    ps = api.PcmStage(0, 1, 4096)
    s = gm.session([q.Utterance(synthetic_prompt(8, 0), q.Speaker.Ryan, q.Language.English, seed=1, max_length=4)],
                   q.SynthesisOptions(max_length=4, seed=1, eos_token_id=None))
    b = _batcher(gm, 1)
    t = b.submit_streamed(_request(gm.config, 0, LIMITS[0]))
    layers = {
        "stage": lambda k, a: (STAGE_FN[k], lambda: getattr(L, STAGE_FN[k])(ps._h, 0, *a)),
        "session": lambda k, a: ("q3_session_set_" + k, lambda: getattr(L, "q3_session_set_" + k)(s._h, *((0,) if k != "output" else ()), *a)),
        "batcher": lambda k, a: ("q3_batcher_ticket_" + k, lambda: getattr(L, "q3_batcher_ticket_" + k)(b._h, t, *a)),
    }
    differ, misnamed = [], []
    try:
        for kind, args, status, first, host in REFUSALS:
            said = {}
            for name, layer in layers.items():
                if first:
                    assert layer(*first)[1]() == 0, (name, first)
                fn, call = layer(kind, args)
                st, who, text = refusal(call)
                if first:                                  # back to the default, which every value admits
                    assert layer(first[0], (1000,))[1]() == 0
                assert st == status, (name, kind, args, st, who, text)
                if who != fn:
                    misnamed.append((fn, args, who))
                said[name] = text
            if host:
                st, who, text = refusal(host)
                assert st == status, (kind, args, st, who, text)
                said["host"] = text
            print(kind, args, said["stage"])
            if len(set(said.values())) != 1:
                differ.append((kind, args, said))
        print("sentences that differ between the layers:", differ)
        print("refusals that name another entry point:", misnamed)
        assert not differ and not misnamed
    finally:
        b.close(); s.close(); ps.close()


# ---------------------------------------------------------------- 2. the whole chain through each layer at once
def full(thr_mb, edge_pause, tempo, cents, target_mb, prior_mb, level):
    """a setting with every step on, as the keyword arguments of api.resample_gpu"""
    return dict(silence=(thr_mb / 100.0,) + tuple(edge_pause), tempo_permille=tempo, pitch_cents=cents, target_mb=target_mb, prior_mb=prior_mb,
                gain_mb=level[0], ceiling_mb=level[1])


def readings(pcm, rate, fmt, kw):
    """the one-shot stage's samples (api.resample_gpu) and, from a stage row set the same way, its loudness reading and silence counts"""
    ps = api.PcmStage(0, 1, max(pcm.size, 1))
    try:
        ps.set(0, rate, fmt=fmt); ps.set_tempo(0, kw["tempo_permille"]); ps.set_pitch(0, kw["pitch_cents"])
        ps.set_level(0, kw["gain_mb"], kw["ceiling_mb"]); ps.set_loudness(0, api.LOUD_NORMALIZE, kw["target_mb"], kw["prior_mb"])
        ps.set_silence(0, *kw["silence"])
        y = ps.push({0: pcm}, last=(0,))[0]
        want = api.resample_gpu(pcm, rate, fmt=fmt, **kw).samples
        assert y.dtype == want.dtype and np.array_equal(y, want)
        return want, tuple(ps.loudness(0)), tuple(ps.silence(0))
    finally:
        ps.close()


def session_set(s, b, kw):
    s.set_silence(*kw["silence"], b=b); s.set_tempo(kw["tempo_permille"], b=b); s.set_pitch(kw["pitch_cents"], b=b)
    s.set_loudness(api.LOUD_NORMALIZE, kw["target_mb"], kw["prior_mb"], b=b); s.set_level(kw["gain_mb"], kw["ceiling_mb"], b=b)


def test_session_rows_run_the_whole_chain(gm):
    """B = 2, chunks of 3 frames, limits 7 and 25, stream mode 1, 8 kHz mu-law. Row 0 has every step on and is replaced, when it
    ends, by an utterance of 8 frames that gets another full setting before its first chunk; row 1 has the shared output alone."""
    opts = q.SynthesisOptions(max_length=25, seed=42, eos_token_id=None, chunk_frames=3)
    new = q.Utterance(synthetic_prompt(9, 77), q.Speaker.Ryan, q.Language.English, seed=5, max_length=8)
    kw, read = {}, {}

    def run(out):
        s = _session(gm, [7, 25], opts, 1)
        if out:
            s.set_output(8000, fmt="ulaw")
            session_set(s, 0, kw["old"])
        parts = {"old": [], "new": [], 1: []}
        key = "old"
        for _ in range(32):
            r = s.next_chunks_out() if out else s.next_chunks()
            for b, (a, _d) in enumerate(r):
                if a is not None:
                    parts[key if b == 0 else b].append(a.samples)
            if r[0][1] and key == "old":
                if out:
                    read["old"] = (tuple(s.loudness(0)), tuple(s.silence(0)))
                s.replace(0, new); key = "new"
                if out:
                    session_set(s, 0, kw["new"])
            elif all(d for _, d in r):
                break
        if out:
            read["new"] = (tuple(s.loudness(0)), tuple(s.silence(0)))
            for fn in (s.loudness, s.silence):
                with pytest.raises(_lib.Q3Error):
                    fn(1)                                  # the row without the steps has no readings
        s.close()
        return {k: _cat(v) for k, v in parts.items()}

    pcm = run(False)
    assert pcm["old"].size == 7 * SPF and pcm["new"].size == 8 * SPF and pcm[1].size == 25 * SPF
    kw["old"] = full(pick(pcm["old"], 0, 20)[0], (0, 20), 1250, -200, -1900, 0, (600, -100))
    kw["new"] = full(pick(pcm["new"], 10, 30)[0], (10, 30), 900, 300, -2300, 300, (-300, -200))
    got = run(True)
    for k in ("old", "new"):
        want, loud, sil = readings(pcm[k], 8000, "ulaw", kw[k])
        assert got[k].dtype == np.uint8 and want.size > 0
        np.testing.assert_array_equal(got[k], want, err_msg=k)
        assert read[k] == (loud, sil), (k, read[k], loud, sil)
        assert sil[1] < sil[0]                             # the silence step cut something
    np.testing.assert_array_equal(got[1], api.resample_gpu(pcm[1], 8000, fmt="ulaw").samples)


def test_batcher_slots_change_between_the_whole_chain_and_none(gm):
    """Two slots, requests 3, 0, 1, 2 of test_batcher_stream.py (27 / 5 / 50 / 20 frames) in that order: slot 0 serves a plain ticket
    and then one with every step on (the stage row's first use comes after the slot's first owner), slot 1 one with every step on —
    it creates the stage — and then a plain one, which never touches the row its predecessor left."""
    order = [3, 0, 1, 2]
    utts = [_request(gm.config, i, LIMITS[i]) for i in order]

    def run(kws):
        b = _batcher(gm, 2)
        tickets = [b.submit_streamed(u, **k) for u, k in zip(utts, kws)]
        got, _ = _drive(b, tickets, {t: True for t in tickets})
        read = [(tuple(b.loudness(t)), tuple(b.silence(t))) if k else None for t, k in zip(tickets, kws)]
        b.close()
        return [_cat(got[t]) for t in tickets], read

    pcm, _ = run([{}, {}, {}, {}])
    assert [p.size for p in pcm] == [LIMITS[i] * SPF for i in order]
    kw = [None, full(pick(pcm[1], 0, 20)[0], (0, 20), 1250, -200, -1900, 0, (600, -100)), None,
          full(pick(pcm[3], 0, 30)[0], (0, 30), 900, 300, -2300, 300, (-300, -200))]
    ends = [None, (8000, "ulaw"), None, (16000, "s16")]

    def ticket_kw(k, end):
        return dict(sample_rate=end[0], fmt=end[1], tempo_permille=k["tempo_permille"], pitch_cents=k["pitch_cents"], gain_mb=k["gain_mb"],
                    ceiling_mb=k["ceiling_mb"], target_lufs=k["target_mb"] / 100.0, prior_gain_db=k["prior_mb"] / 100.0, silence=k["silence"])
    got, read = run([ticket_kw(k, e) if k else {} for k, e in zip(kw, ends)])
    for i in range(4):
        if kw[i] is None:
            np.testing.assert_array_equal(got[i].view(np.uint32), pcm[i].view(np.uint32), err_msg=f"request {order[i]}")
            continue
        want, loud, sil = readings(pcm[i], *ends[i], kw[i])
        assert got[i].dtype == want.dtype and want.size > 0
        np.testing.assert_array_equal(got[i], want, err_msg=f"request {order[i]}")
        assert read[i] == (loud, sil), (order[i], read[i], loud, sil)


# ---------------------------------------------------------------- 3. a reused stage row
def test_a_reused_row_does_not_depend_on_the_setter_order():
    """Row 0 is fresh and set in the documented order; row 1 has had another setting and a whole stream, and reaches the same
    setting from the other end. Pitch -300 is not admissible at the tempo row 1 still has (2000 would need the stretcher at 2378):
    that call is refused and leaves the row as it is, in the middle of a stream; after the tempo it is accepted."""
    x = X[:12000]
    ps = api.PcmStage(0, 2, 1 << 16)
    try:
        ps.set(0, 16000, fmt="s16"); ps.set_tempo(0, 800); ps.set_pitch(0, -300); ps.set_level(0, 600, -100)
        ps.set(1, 48000); ps.set_tempo(1, 2000); ps.set_silence(1, -50.0, 20, 40); ps.set_loudness(1, api.LOUD_NORMALIZE)
        assert ps.push({1: x}, last=(1,))[1].size > 0
        ps.set_level(1, 600, -100)
        ps.push({1: x[:4800]})                             # the row is in the middle of a stream again
        before = (tuple(ps.loudness(1)), tuple(ps.silence(1)))
        assert before[1][0] == 4800
        with pytest.raises(_lib.Q3Error) as e:
            ps.set_pitch(1, -300)
        assert e.value.status == Q3_INVALID_ARG and "2378" in str(e.value)
        assert (tuple(ps.loudness(1)), tuple(ps.silence(1))) == before and ps._pitch[1] == 0      # neither restarted nor changed
        ps.set_tempo(1, 800); ps.set_pitch(1, -300); ps.set(1, 16000, fmt="s16")
        ps.set_silence(1, None); ps.set_loudness(1, api.LOUD_OFF)
        got = {0: [], 1: []}
        sizes = push_sizes(x.size, 4801)
        at = 0
        for k, n in enumerate(sizes):
            out = ps.push({0: x[at:at + n], 1: x[at:at + n]}, last=(0, 1) if k == len(sizes) - 1 else ())
            at += n
            for r in (0, 1):
                got[r].append(out[r])
        a, b = np.concatenate(got[0]), np.concatenate(got[1])
        assert a.dtype == np.int16 and a.size > 0
        np.testing.assert_array_equal(a, b)
    finally:
        ps.close()
