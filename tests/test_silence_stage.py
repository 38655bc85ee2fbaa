"""The output stage's silence step on the device (k_trim): edges trimmed and pauses capped at the very front of a
row. The reference is the numpy float32 restatement of test_silence_host.py and every sample comparison is bitwise; the counts per
push are those of its streaming rule. Synthetic PCM, no model."""
import math

import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
from test_silence_host import (FS, G, H, bits, case, hold_np, hops_of, make_signal, push_sizes, restate, stream_counts)

pytestmark = pytest.mark.gpu
SETTING = (-5000, 50, 400)                                 # E = 5, P = 40: the "main" signal is 253 hops and 100 samples
CUTS = [1, 239, 240, 241, 479, 1920, 5000, 19200]
ONE = (-5000, 20, 40)                                     # single-sample pushes: a short signal of its own, whole (E = 2, P = 4, P1 = P2 = 2)
Q3_INVALID_ARG = 1
f32 = np.float32


def db(setting):
    return setting[0] / 100.0, setting[1], setting[2]


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, 1 << 20)
    yield ps
    ps.close()


def fresh(ps, row, setting=None, rate=24000, fmt="f32", tempo=1000, level=(0, 0), loud=None):
    ps.set(row, rate, fmt=fmt)
    ps.set_pitch(row, 0); ps.set_tempo(row, tempo); ps.set_level(row, *level)
    ps.set_loudness(row, api.LOUD_NORMALIZE if loud else api.LOUD_OFF, *(loud or (-1900, 0)))
    if setting is None:
        ps.set_silence(row, None, 0, 20)
    else:
        ps.set_silence(row, *db(setting))


def run_row(ps, row, x, sizes):
    outs = []; at = 0
    for k, n in enumerate(sizes):
        last = k == len(sizes) - 1
        outs.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
    return outs


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.size == b.size and (a.view(np.uint8) == b.view(np.uint8)).all()


def emitted_8k(n, ended):
    """the resampler's streaming rule at 8 kHz (L / M = 1 / 3) after n samples of its input"""
    if ended:
        return int(math.floor(n * (8000.0 / 24000.0) + 0.5))
    return (n - 64 + 2) // 3 if n > 64 else 0


@pytest.fixture(scope="module")
def one_push(stage):
    """the device's one-push outputs of the main signal at f32 / 24 kHz and mu-law / 8 kHz, computed once"""
    x = case("main", SETTING)[0]
    res = {}
    for key, rate, fmt in (("f32", 24000, "f32"), ("ulaw", 8000, "ulaw")):
        fresh(stage, 0, SETTING, rate, fmt)
        y = stage.push({0: x}, last=(0,))[0]
        y.setflags(write=False)
        res[key] = (y, stage.silence(0))
    return res


def test_one_push_is_the_restatement(stage, one_push):
    x, y, counts, ops, need, act = case("main", SETTING)
    got, reading = one_push["f32"]
    assert got.size == y.size and (bits(got) == bits(y)).all()
    assert tuple(reading) == counts and reading.n_in - reading.lead_cut - reading.pause_cut - reading.trail_cut == reading.n_out
    assert reading.lead_cut > 0 and reading.pause_cut > 0 and reading.trail_cut > 0
    assert one_push["ulaw"][0].size == emitted_8k(y.size, True) and tuple(one_push["ulaw"][1]) == counts
    for name in ("zeros", "active_ends", "silent", "short_silent"):
        x2, y2, c2 = case(name, SETTING)[:3]
        fresh(stage, 1, SETTING)
        got = stage.push({1: x2}, last=(1,))[1]
        assert got.size == y2.size and (bits(got) == bits(y2)).all(), name
        assert tuple(stage.silence(1)) == c2, name


@pytest.mark.parametrize("cut", CUTS)
@pytest.mark.parametrize("fmt", ["f32", "ulaw"])
def test_every_cut_returns_the_bits_of_one_push_and_the_counts_of_the_rule(stage, one_push, cut, fmt):
    x, y, counts, ops, need, act = case("main", SETTING)
    setting = SETTING
    if cut == 1:
        # one launch per sample: a signal of 27 hops and 37 samples, whole — a leading cut, a hop that leaves at once, the head
        # carried from push to push, a seam (a run of P + 3 hops), a trailing cut and a partial last hop
        setting = ONE
        E, P = hops_of(*ONE[1:])[:2]
        x = make_signal([("Q", E + 1 + G), ("S", 3), ("Q", P + 3 + 2 * G), ("S", 2), ("Q", E + 2 + G)], ONE[0], 31, tail=37)
        y, counts, ops, need = restate(x, *ONE)
        assert counts[2] > 0 and counts[3] > 0 and counts[4] > 0 and any(b >= 0 for _, b in ops)
        fresh(stage, 1, ONE, 8000 if fmt == "ulaw" else 24000, fmt)
        want = stage.push({1: x}, last=(1,))[1]
        if fmt == "f32":
            assert want.size == y.size and (bits(want) == bits(y)).all()
    else:
        want = one_push[fmt][0]
    sizes = push_sizes(x.size, cut)
    fresh(stage, 0, setting, 8000 if fmt == "ulaw" else 24000, fmt)
    outs = run_row(stage, 0, x, sizes)
    assert same(np.concatenate(outs), want)
    kept = stream_counts(need, counts, sizes)
    if fmt == "ulaw":
        tot = np.cumsum(kept)
        em = [emitted_8k(int(t), k == len(sizes) - 1) for k, t in enumerate(tot)]
        kept = np.diff(np.concatenate([[0], em]))
    assert [o.size for o in outs] == kept.tolist()
    assert tuple(stage.silence(0)) == counts


def test_off_is_a_row_that_was_never_set(one_push):
    x = case("main", SETTING)[0]
    a = api.PcmStage(0, 2, x.size)
    try:
        for row in (0, 1):
            a.set(row, 16000, fmt="s16"); a.set_tempo(row, 1250)
        a.set_silence(1, -50.0, 50, 400); a.set_silence(1, None, 50, 400)      # on, then off
        sizes = push_sizes(x.size, 19200)
        o0 = run_row(a, 0, x, sizes); o1 = run_row(a, 1, x, sizes)
        assert [o.size for o in o0] == [o.size for o in o1] and same(np.concatenate(o0), np.concatenate(o1))
        with pytest.raises(_lib.Q3Error):
            a.silence(1)
        assert _lib.lib.q3_pcm_stage_set_silence(a._h, 0, -5000, 55, 400) == Q3_INVALID_ARG
        assert _lib.lib.q3_pcm_stage_set_silence(a._h, 0, -1000, 50, 400) == Q3_INVALID_ARG
        assert _lib.lib.q3_pcm_stage_set_silence(a._h, 2, -5000, 50, 400) == Q3_INVALID_ARG
    finally:
        a.close()


def test_three_rows_with_their_own_settings_and_push_sizes(stage):
    rows = {0: ((-5000, 50, 400), "main", 1920), 1: ((-5000, 0, 20), "main", 5000), 2: ((-4000, 100, 200), "active_ends", 777)}
    xs, ys, at, outs = {}, {}, {}, {}
    for r, (setting, name, cut) in rows.items():
        xs[r], ys[r] = case(name, setting)[:2]
        fresh(stage, r, setting)
        at[r] = 0; outs[r] = []
    while at:
        batch = {r: xs[r][at[r]:at[r] + rows[r][2]] for r in at}
        last = tuple(r for r in at if at[r] + rows[r][2] >= xs[r].size)
        got = stage.push(batch, last=last)
        for r in list(at):
            outs[r].append(got[r]); at[r] += rows[r][2]
            if r in last:
                del at[r]
    for r, (setting, name, cut) in rows.items():
        y = np.concatenate(outs[r])
        assert y.size == ys[r].size and (bits(y) == bits(ys[r])).all(), r
        assert tuple(stage.silence(r)) == case(name, setting)[2], r


def test_non_finite_samples_in_kept_and_dropped_hops(stage):
    E, P, P1, P2 = hops_of(*SETTING[1:])
    x = case("main", SETTING)[0].copy()
    burst = (E + 1 + G + 2) * H
    x[burst + 7] = np.nan; x[burst + H + 9] = np.inf          # inside the first burst: kept, and 0 for the energy
    x[3] = np.nan; x[H + 1] = -np.inf                         # the leading run of E + 1 hops: in its dropped hop, and in its kept edge
    long_run = (E + 1 + G + 5 + P + 2 * G + 3 + G) * H        # the run of P + 1 hops: its one dropped hop is the seam's partner
    x[long_run + P1 * H + 5] = np.inf
    x[long_run + (P1 - 1) * H + 11] = np.nan
    y, counts, ops, need = restate(x, *SETTING)
    # kept as they are: the burst's two and the edge's one; through the seam: its own NaN and its partner's infinity
    assert np.isnan(y).sum() == 2 and np.isinf(y).sum() == 3
    for cut in (x.size, 1920):
        fresh(stage, 0, SETTING)
        got = np.concatenate(run_row(stage, 0, x, push_sizes(x.size, cut)))
        assert got.size == y.size and (bits(got) == bits(y)).all(), cut
        assert tuple(stage.silence(0)) == counts


def test_a_refused_push_leaves_the_row_where_it_was(stage):
    x, y, counts = case("main", SETTING)[:3]
    fresh(stage, 0, SETTING)
    sizes = push_sizes(x.size, 5000)
    outs = []; at = 0
    for k, n in enumerate(sizes):
        last = k == len(sizes) - 1
        if k in (2, 5, len(sizes) - 1):
            before = stage.silence(0)
            with pytest.raises(_lib.Q3Error):               # the cap has to cover the a-priori bound, whatever would come
                stage._push_lists([0], [x[at:at + n]], [last], cap=[stage.bound(0, n) - 1])
            assert stage.silence(0) == before
        outs.append(stage.push({0: x[at:at + n]}, last=(0,) if last else ())[0])
        at += n
    got = np.concatenate(outs)
    assert got.size == y.size and (bits(got) == bits(y)).all() and tuple(stage.silence(0)) == counts
    with pytest.raises(_lib.Q3Error):                       # flushed: restarted by set / reset only
        stage.push({0: x[:10]})
    small = api.PcmStage(0, 1, 1000)                        # max_push_samples applies to what enters the step
    try:
        small.set_silence(0, -50.0, 50, 400)
        assert small.push({0: x[:1000]})[0].size <= 1000
        with pytest.raises(_lib.Q3Error):
            small.push({0: x[:1001]})
    finally:
        small.close()


def test_thirty_seconds_of_silence_between_two_bursts(stage):
    """The row's state is allocated by set_silence and k_trim cannot grow it: a run far longer than hold is served from the bounded
    retention alone. No push returns more than its own samples and hold, and none during the run returns anything."""
    setting = (-5000, 50, 400)
    x = make_signal([("S", 30), ("Q", 3000), ("S", 30)], setting[0], 21, tail=123)
    y, counts, ops, need = restate(x, *setting)
    assert counts[3] == (3000 - 2 * G - 40) * H
    fresh(stage, 0, setting)
    sizes = push_sizes(x.size, 19200)
    outs = run_row(stage, 0, x, sizes)
    got = np.concatenate(outs)
    assert got.size == y.size and (bits(got) == bits(y)).all() and tuple(stage.silence(0)) == counts
    assert [o.size for o in outs] == stream_counts(need, counts, sizes).tolist()
    assert all(o.size <= n + hold_np(*setting[1:]) for o, n in zip(outs, sizes))
    assert sum(o.size == 0 for o in outs) >= 3000 * H // 19200 - 3


def test_composition_with_the_steps_behind(stage):
    """tempo 1250, level (+600, -100), loudness normalise, 16 kHz s16: the row with the step on, fed x in pushes, against the same
    steps as a one-shot row fed the restated y"""
    x, y = case("main", SETTING)[:2]
    kw = dict(rate=16000, fmt="s16", tempo=1250, level=(600, -100), loud=(-1900, 0))
    fresh(stage, 1, None, **kw)
    want = stage.push({1: y}, last=(1,))[1]
    for cut in (19200, 1920):
        fresh(stage, 0, SETTING, **kw)
        outs = run_row(stage, 0, x, push_sizes(x.size, cut))
        assert same(np.concatenate(outs), want), cut
        assert all(o.size <= stage.bound(0, cut) for o in outs)
    assert want.size > 0 and want.dtype == np.int16


def test_set_and_reset_keep_the_setting(stage):
    x, y, counts = case("main", SETTING)[:3]
    fresh(stage, 0, SETTING)
    stage.push({0: x[:30000]})
    stage.reset(0)                                          # restarts the row; the step stays
    got = stage.push({0: x}, last=(0,))[0]
    assert (bits(got) == bits(y)).all()
    stage.set(0, 8000, fmt="ulaw"); stage.set_tempo(0, 1000); stage.set_level(0, 0, 0)
    got = stage.push({0: x}, last=(0,))[0]
    assert got.dtype == np.uint8 and got.size == emitted_8k(y.size, True) and tuple(stage.silence(0)) == counts
    assert tuple(stage.silence(0))[0] == x.size
