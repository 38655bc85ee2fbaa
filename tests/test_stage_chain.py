"""The output stage's chain: silence -> stretcher / pitch -> loudness -> level -> resampler / format. A row's chain is the
composition of its steps, and pushes may cut the stream anywhere: every one of the 32 chains, at two ends (24 kHz f32 and 8 kHz
mu-law), fed in pushes on one row, returns BITWISE what the same steps return as single-unit rows, each run alone at 24 kHz f32 in
one push with `last` (where the resampler is a copy: test_24k_f32_is_a_copy) and fed to the next, the format end last. The tempo
and the pitch are one unit: the stretcher runs at the effective tempo, so the two do not decompose further. Four rows run per
push, each with its own chain and its own cut, and some pushes give a row no samples. Synthetic PCM, no model."""
import functools

import numpy as np
import pytest

from qwen3_tts_rs_amd import api
from test_silence_host import G, H, hold_np, hops_of, make_signal, push_sizes

pytestmark = pytest.mark.gpu
SILENCE = (-5000, 20, 40)                                  # E = 2, P = 4: a row retains at most 1 920 samples
TEMPO_PITCH = [(1000, 0), (1250, 0), (1000, 300), (1250, -200)]      # off, tempo only, pitch only (the stretcher at 841), both (at 1403)
LOUD, LEVEL = (-1900, 0), (600, -100)
ENDS = [(24000, "f32"), (8000, "ulaw")]
CUTS = [1920, 1001, 4801, 9600]                            # the silence step's hold, an odd one, and two that are no multiple of a hop or a tile
# Cases whose single-unit composition did not hold bitwise on the commit before this test: they compare against the same chain in
# one push on a fresh row instead (chunk invariance only). At most 4; each with its reason.
ONE_PUSH_ONLY = {}


def the_signal():
    """0.91 s: a leading run, two pauses longer than the cap, a trailing run and a ragged last hop; longer than every step's
    hold-back (64, 64, 127, the stretcher's 720 + 240, 1 920)"""
    E, P = hops_of(*SILENCE[1:])[:2]
    spec = [("Q", E + 6), ("S", 15), ("Q", P + 3 + 2 * G), ("S", 20), ("Q", P + 5 + 2 * G), ("S", 18), ("Q", E + 2 + G)]
    x = make_signal(spec, SILENCE[0], 47, tail=37)
    x.setflags(write=False)
    return x


X = the_signal()


def chain_of(g, r):
    """row r of group g (0 .. 7): (silence, tempo / pitch unit, loudness, level). The four rows of a group differ in every unit."""
    return (g >> 2 & 1) ^ (r in (1, 2)), r, (g >> 1 & 1) ^ (r >> 1), (g & 1) ^ (r & 1)


CASES = [(g, r) for g in range(16) for r in range(4)]      # groups 8 .. 15: the chains of 0 .. 7 at the other end


def end_of(g, r):
    return ENDS[(r + g // 8) % 2]


def case_id(c):
    sil, tp, loud, level = chain_of(c[0] % 8, c[1])
    return "-".join(["sil" if sil else "0", ["0", "tempo", "pitch", "both"][tp], "loud" if loud else "0", "level" if level else "0",
                     end_of(*c)[1]])


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, 1 << 16)
    yield ps
    ps.close()


def configure(ps, row, sil=0, tp=0, loud=0, level=0, end=ENDS[0]):
    ps.set(row, end[0], fmt=end[1])
    ps.set_pitch(row, 0); ps.set_tempo(row, TEMPO_PITCH[tp][0]); ps.set_pitch(row, TEMPO_PITCH[tp][1])
    ps.set_level(row, *(LEVEL if level else (0, 0)))
    ps.set_loudness(row, api.LOUD_NORMALIZE if loud else api.LOUD_OFF, *LOUD)
    ps.set_silence(row, SILENCE[0] / 100.0 if sil else None, *SILENCE[1:])


def same(a, b):
    a = np.asarray(a); b = np.asarray(b)
    return a.dtype == b.dtype and a.size == b.size and (a.view(np.uint8) == b.view(np.uint8)).all()


def unit_runner(ps):
    """the stream behind the first k units of a chain, each unit a row of its own in one push; computed once per prefix"""
    @functools.lru_cache(maxsize=None)
    def behind(prefix):
        if not prefix:
            return X
        x = behind(prefix[:-1])
        k, v = len(prefix) - 1, prefix[-1]
        if not v or (k == 4 and v == ENDS[0]):             # (the step is off; at 24 kHz f32 the end is a copy)
            return x
        configure(ps, 0, **{("sil", "tp", "loud", "level", "end")[k]: v})
        y = ps.push({0: x}, last=(0,))[0]
        assert y.size > 0
        y.setflags(write=False)
        return y
    return behind


@pytest.fixture(scope="module")
def expected(stage):
    return unit_runner(stage)


@pytest.fixture(scope="module")
def pushed(stage):
    """the four rows of a group, fed in pushes: per row the pieces that came out and, per push, (samples in, samples out, bound)"""
    @functools.lru_cache(maxsize=None)
    def run(g):
        plan = {}
        for r in range(4):
            configure(stage, r, *chain_of(g % 8, r), end=end_of(g, r))
            sizes = push_sizes(X.size, CUTS[(r + g) % 4])
            for at in (1 + r % 2, 4 + r):                  # pushes that give the row nothing
                if at < len(sizes):
                    sizes.insert(at, 0)
            plan[r] = sizes
        outs = {r: [] for r in plan}; log = {r: [] for r in plan}; at = {r: 0 for r in plan}
        k = 0
        while any(k < len(s) for s in plan.values()):
            rows = [r for r in plan if k < len(plan[r])]
            batch = {r: X[at[r]:at[r] + plan[r][k]] for r in rows}
            got = stage.push(batch, last=tuple(r for r in rows if k == len(plan[r]) - 1))
            for r in rows:
                outs[r].append(got[r]); log[r].append((plan[r][k], got[r].size, stage.bound(r, plan[r][k])))
                at[r] += plan[r][k]
            k += 1
        assert all(at[r] == X.size for r in plan)
        return outs, log
    return run


def test_the_cases_are_the_32_chains_at_two_ends():
    assert len({chain_of(g, r) for g in range(8) for r in range(4)}) == 32
    assert len({(chain_of(g % 8, r), end_of(g, r)) for g, r in CASES}) == 64
    assert all(len({chain_of(g, r)[u] for r in range(4)}) > 1 for g in range(8) for u in range(4))
    assert 1920 in CUTS and hold_np(*SILENCE[1:]) == 1920 and any(c % 2 for c in CUTS)
    assert 12000 <= X.size <= 24000 and X.size % H != 0
    assert len(ONE_PUSH_ONLY) <= 4


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_a_chain_in_pushes_is_the_composition_of_its_units(stage, expected, pushed, case):
    g, r = case
    chain, end = chain_of(g % 8, r), end_of(g, r)
    outs, log = pushed(g)
    if case_id(case) in ONE_PUSH_ONLY:
        configure(stage, 0, *chain, end=end)
        want = stage.push({0: X}, last=(0,))[0]
    else:
        want = expected(chain + (end,))
    got = np.concatenate(outs[r])
    assert want.size > 0 and same(got, want)
    assert any(n == 0 for n, _, _ in log[r]) and all(m <= b for _, m, b in log[r])
