"""The formant step on the GPU: k_fm_frame / k_fm_ola against the float64 restatement (formant_cases.formant_ref)
of what the step in front hands it, split invariance bit for bit, rows with the step off, and a session row.

The largest absolute errors measured over the stage-level cases below were 1.54e-6, 6.92e-6, 6.7e-7 and 1.36e-6 in the order of the
table (signal peak 0.25, a gain of up to 18 dB); BOUND is four times the largest, as DESIGN 4.12g records."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from test_output_format import _session
import formant_cases as fc

pytestmark = pytest.mark.gpu
BOUND = 4 * 6.92e-6
LENGTHS = (1023, 1024, 1025, 6000)       # first frame alone, an exact frame, one sample into the next, a tail


@pytest.fixture(scope="module")
def probe():
    x = fc.vowel()
    x.setflags(write=False)
    return x


def _stage(rows, cents=0, formant=None, plain=()):
    ps = api.PcmStage(0, rows, 8192)
    for r in range(rows):
        if cents:
            ps.set_pitch(r, cents)
        if formant is not None and r not in plain:
            ps.set_formant(r, *formant)
    return ps


@pytest.mark.parametrize("cents,keep,fcents", [(400, 1, 0), (-300, 1, 0), (0, 0, 200), (400, 1, -200)])
def test_stage_against_float64(probe, cents, keep, fcents):
    """Rows 0..3 with the step, rows 4..7 without: one push, one launch set. The reference is formant_ref of what the twin row delivers."""
    omega, runs = api.pcm_stage_formant_plan(1000, cents, keep, fcents)
    assert runs
    ps = _stage(8, cents, (keep, fcents), plain=(4, 5, 6, 7))
    out = ps.push({r: probe[:LENGTHS[r % 4]] for r in range(8)}, last=range(8))
    ps.close()
    worst = 0.0
    for r, n in enumerate(LENGTHS):
        v = out[4 + r]
        assert out[r].size == v.size and (cents != 0 or np.array_equal(v, probe[:n]))
        worst = max(worst, float(np.abs(out[r] - fc.formant_ref(v, omega)).max()))
        assert not np.array_equal(out[r], v)
    print(f"({cents}, {keep}, {fcents}): omega {omega}, largest absolute error {worst:.3e}")
    assert worst <= BOUND


def test_split_invariance_and_a_refused_push(probe):
    x = probe[:6000]
    ps = _stage(2, 0, (0, 200))                                # (the step alone: what a push returns follows from its rule)
    whole = ps.push({0: x}, last=(0,))[0]
    parts = []
    for k, (a, b) in enumerate(((0, 1), (1, 256), (256, 1025), (1025, 6000))):
        if k == 2:                                             # 256 samples are due: a buffer for none is refused, the row stays
            with pytest.raises(_lib.Q3Error) as e:
                ps._push_lists([1], [x[a:b]], [False], cap=[0])
            assert e.value.status == 1
        parts.append(ps.push({1: x[a:b]}, last=(1,) if b == 6000 else ())[1])
    ps.close()
    assert [p.size for p in parts] == [0, 0, 256, 5744]
    np.testing.assert_array_equal(np.concatenate(parts), whole)


def test_off_means_off(probe):
    """keep = 0, fcents = 0 — and keep = 1 on a row without a pitch — beside a row with the step on: the bits of a stage that never
    saw set_formant."""
    x = probe[:6000]
    ps = api.PcmStage(0, 3, 8192)
    ps.set_pitch(0, 400); ps.set_formant(0, False, 0); ps.set_formant(1, True, 0); ps.set_pitch(2, 400); ps.set_formant(2, True, 0)
    got = ps.push({0: x, 1: x, 2: x}, last=(0, 1, 2))
    ps.close()
    ps = _stage(1, 400)
    want = ps.push({0: x}, last=(0,))[0]
    ps.close()
    np.testing.assert_array_equal(got[0], want)
    np.testing.assert_array_equal(got[1], x)
    assert not np.array_equal(got[2], want)


def test_session_row():
    """B = 2 through next_chunks_out: row 0 at +300 cents with keep, row 1 plain. Row 1 is, chunk for chunk, the session that never
    heard of the setting; row 0 is the one-shot stage on the PCM the same session delivers without it."""
    gm = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    opts = q.SynthesisOptions(max_length=12, seed=42, eos_token_id=None, chunk_frames=3)

    def run(kind):
        s = _session(gm, [7, 12], opts, 1)
        if kind == "formant":
            for bad in ((True, 601, 0), (True, 0, 2)):
                with pytest.raises(_lib.Q3Error):
                    s.set_formant(*bad)
            s.set_pitch(300, 0); s.set_formant(True, 0, 0)
        parts = [[], []]
        for _ in range(16):
            r = s.next_chunks() if kind == "pcm" else s.next_chunks_out()
            for b, (a, d) in enumerate(r):
                if a is not None:
                    parts[b].append(a.samples)
            if all(d for _, d in r):
                break
        s.close()
        return parts
    got, pcm, plain = run("formant"), run("pcm"), run("plain")
    gm.close()
    assert len(got[1]) == len(plain[1]) and all(np.array_equal(a, w) for a, w in zip(got[1], plain[1]))
    want = api.resample_gpu(np.concatenate(pcm[0]), 24000, pitch_cents=300, formant=(True, 0)).samples
    np.testing.assert_array_equal(np.concatenate(got[0]), want)
    assert not np.array_equal(want, api.resample_gpu(np.concatenate(pcm[0]), 24000, pitch_cents=300).samples)
