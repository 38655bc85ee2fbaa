"""The tone step on the GPU: k_tone against the sequential float64 cascade (tone_cases.cascade). The tolerance is
measured per case: twice what the same cascade run sequentially in float32 deviates from float64, plus one f32 ulp of the peak
(tone_cases.tolerance) — the factor 2 for the sums the scan reorders. DESIGN 4.12h records both figures per case."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from test_batcher_stream import LIMITS, OPTS, STEP, _request
import tone_cases as tc

pytestmark = pytest.mark.gpu
LENGTHS = (1, 63, 64, 65, 4095, 4096, 4097, 9000)             # a segment's edge, a wave's edge, the loop, a ragged last segment


@pytest.fixture(scope="module")
def refs():
    """per band set the float64 and the float32 cascade of the whole signal: a causal filter's first n outputs are those of x[:n]"""
    x = tc.signal()
    x.setflags(write=False)
    return x, {k: (tc.cascade(x, b), tc.cascade(x, b, np.float32)) for k, b in tc.SETS.items()}


def _check(got, r64, r32, what):
    err, tol = float(np.abs(got.astype(np.float64) - r64).max()), tc.tolerance(r64, r32)
    print(f"{what}: float32 recursion {np.abs(r32.astype(np.float64) - r64).max():.3e}, k_tone {err:.3e}, tolerance {tol:.3e}")
    assert got.dtype == np.float32 and got.size == r64.size and err <= tol, what


@pytest.mark.parametrize("name", sorted(tc.SETS))
def test_against_float64(refs, name):
    """Eight rows, one per length, in one push: one launch, a workgroup per row."""
    x, ref = refs
    ps = api.PcmStage(0, len(LENGTHS), 9000)
    for r in range(len(LENGTHS)):
        ps.set_tone(r, tc.SETS[name])
    out = ps.push({r: x[:n] for r, n in enumerate(LENGTHS)})
    ps.close()
    for r, n in enumerate(LENGTHS):
        _check(out[r], ref[name][0][:n], ref[name][1][:n], f"{name} n = {n}")


def test_cuts_rows_and_refusals(refs):
    """Row 0: the full cascade in pieces; row 1: no bands, beside it in the same pushes; row 2: another set in other pieces. The
    same cuts again give the same bits; a setting out of range leaves the row as it was."""
    x, ref = refs
    cuts = {0: (1, 63, 65, 1920, 4097, 2854), 1: (9000, 0, 0, 0, 0, 0), 2: (4096, 64, 4840, 0, 0, 0)}

    def run():
        ps = api.PcmStage(0, 3, 9000)
        ps.set_tone(0, tc.FULL); ps.set_tone(1, tc.PEAK); ps.set_tone(1, None); ps.set_tone(2, tc.HP20)
        for bad, word in ((tc.FULL + tc.PEAK, "n_bands"), ([("peak", 12000)], "freq_hz")):
            with pytest.raises(_lib.Q3Error, match=word):
                ps.set_tone(2, bad)
        at, parts = {r: 0 for r in cuts}, {r: [] for r in cuts}
        for k in range(6):
            push = {r: x[at[r]:at[r] + c[k]] for r, c in cuts.items() if c[k]}
            for r, a in ps.push(push).items():
                parts[r].append(a); at[r] += a.size
        ps.close()
        return {r: np.concatenate(p) for r, p in parts.items()}
    got, again = run(), run()
    _check(got[0], *ref["full"], "full in six pieces")
    _check(got[2], *ref["hp20"], "hp20 in three pieces")
    np.testing.assert_array_equal(got[1], x)
    for r in cuts:
        np.testing.assert_array_equal(got[r].view(np.uint32), again[r].view(np.uint32))


def test_a_parked_and_resumed_ticket():
    """A streamed ticket with a tone, parked in slot 0 and resumed in slot 1: its stage row and the sections' states follow it."""
    bands = [("hp", 120), ("peak", 3000, 6.0, 4.0)]
    gm = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    utts = [_request(gm.config, i, LIMITS[i]) for i in range(3)]

    def run(park, tone):
        b = q.Batcher(gm, slots=2, frame_budget=70, prompt_budget=48, options=q.SynthesisOptions(**OPTS), **(dict(max_parked=2) if park else {}))
        S = b.submit_streamed(utts[1], tone=tone)                          # 50 frames
        b.submit(utts[0], want_pcm=False)
        b.step(STEP)
        got = [b.read(S)[0]]
        if park:
            b.park(S); b.submit(utts[2], want_pcm=False); b.step(1); b.unpark(S); b.step(1)
        for _ in range(400):
            running, queued, _f = b.step(STEP)
            got.append(b.read(S)[0])
            if running == 0 and queued == 0:
                break
        a, done = b.read(S); got.append(a)
        assert done and (not park or b.park_info()["moved"] == 1)
        b.close()
        return np.concatenate([g for g in got if g.size])
    pcm, straight, parked = run(False, None), run(False, bands), run(True, bands)
    gm.close()
    r64, r32 = tc.cascade(pcm, bands), tc.cascade(pcm, bands, np.float32)
    _check(straight, r64, r32, "ticket")
    _check(parked, r64, r32, "ticket, parked and resumed")
    assert not np.array_equal(straight, pcm)
