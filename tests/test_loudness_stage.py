"""The output stage's loudness step on the device (k_loud): a BS.1770-4 meter per row and a causal normaliser in
front of the level. The reference is the numpy float32 restatement of test_loudness_host.py and every comparison is bitwise; the
readings meet the float64 fixture within that file's allowance. Synthetic PCM, no model."""
import numpy as np
import pytest

from qwen3_tts_rs_amd import _lib, api
from test_loudness_host import (FS, GOLDEN, HIST, HOP, SIGNALS, TOL_LU, consts_np, gate, k_energies, lufs, normalise, reference, track)

pytestmark = pytest.mark.gpu
CUTS = [1, 63, 64, 65, 1920, 2399, 2400, 2401, 5000, 19200]
N_SIG = 9 * HOP + 877                                      # nine hops and a part of the tenth: six blocks
TARGET = -1900
Q3_INVALID_ARG = 1
f32 = np.float32
OFF, METER, NORM = api.LOUD_OFF, api.LOUD_METER, api.LOUD_NORMALIZE


def signal(n=N_SIG, seed=5, level=0.06):
    """noise under a slow envelope, near -25 LUFS, never silent"""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    return (level * (0.35 + 0.65 * np.abs(np.sin(2.0 * np.pi * 1.7 * t + 0.3))) * rng.standard_normal(n)).astype(f32)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.fixture(scope="module")
def sig():
    x = signal()
    x.setflags(write=False)
    return x


@pytest.fixture(scope="module")
def want(sig):
    """the restatement of the signal at (-1900, 0) and at (-2300, +600), computed once: {(target, prior): (y, z, Ms, As, cg)}"""
    e = k_energies(sig[None, :])[0]
    res = {}
    for target, prior in ((TARGET, 0), (-2300, 600)):
        z, Ms, As, cg = track(e, target, prior)
        y = normalise(sig, As, prior)
        for a in (y, z, Ms, As):
            a.setflags(write=False)
        res[(target, prior)] = (y, z, Ms, As, cg)
    return res


@pytest.fixture(scope="module")
def stage():
    ps = api.PcmStage(0, 4, N_SIG)
    yield ps
    ps.close()


def run_row(ps, row, x, piece):
    out = []; at = 0
    while True:
        n = min(piece, x.size - at); last = at + n >= x.size
        out.append(ps.push({row: x[at:at + n]}, last=(row,) if last else ())[row])
        at += n
        if last:
            return out


def check_reading(r, z, Ms, As, cg):
    assert r.blocks == z.size and r.gated == cg
    assert bits(f32(r.mean_square)) == bits(Ms[-1]) and bits(f32(r.gain)) == bits(As[-1]), (r, Ms[-1], As[-1])


def test_one_push_equals_the_restatement(stage, sig, want):
    y, z, Ms, As, cg = want[(TARGET, 0)]
    T, P, ga, lo, hi = consts_np(TARGET, 0)
    print(f"{z.size} blocks, {cg} gated, {lufs(Ms[-1]):.3f} LUFS, gains {20 * np.log10(As.astype(float)).min():.2f} .. {20 * np.log10(As.astype(float)).max():.2f} dB")
    assert z.size == 6 and np.all(As[3:] > lo) and np.all(As[3:] < hi) and len(set(As[3:].tolist())) == 6      # the gain moves and rests inside its bounds
    stage.set(0, 24000); stage.set_loudness(0, NORM, TARGET, 0)
    assert stage.loudness(0) == api.Loudness.of(0.0, 1.0, 0, 0) and stage.loudness_blocks(0).size == 0
    got = run_row(stage, 0, sig, sig.size)[0]
    assert got.dtype == np.float32 and got.size == sig.size
    bad = np.flatnonzero(bits(got) != bits(y))
    assert bad.size == 0, (bad.size, int(bad[0]), float(got[bad[0]]), float(y[bad[0]]))
    assert np.array_equal(bits(stage.loudness_blocks(0)), bits(z))
    check_reading(stage.loudness(0), z, Ms, As, cg)
    assert abs(stage.loudness(0).lufs - lufs(Ms[-1])) < 1e-9
    # another target and a prior: the first 400 ms leave at the prior
    y2, z2, Ms2, As2, cg2 = want[(-2300, 600)]
    stage.set_loudness(0, NORM, -2300, 600)
    got = run_row(stage, 0, sig, sig.size)[0]
    assert np.array_equal(bits(got), bits(y2)) and np.array_equal(bits(got[:4 * HOP]), bits(sig[:4 * HOP] * consts_np(-2300, 600)[1]))
    check_reading(stage.loudness(0), z2, Ms2, As2, cg2)


@pytest.fixture(scope="module")
def whole(stage, sig):
    """One push of the whole signal at (-1900, 0): (24 kHz f32, 8 kHz ulaw) — computed once, read by the tests below."""
    stage.set(0, 24000); stage.set_loudness(0, NORM, TARGET, 0)
    a = run_row(stage, 0, sig, sig.size)[0]
    stage.set(0, 8000, fmt="ulaw")
    b = run_row(stage, 0, sig, sig.size)[0]
    a.setflags(write=False); b.setflags(write=False)
    return a, b


@pytest.mark.parametrize("cut", CUTS)
def test_cut_invariance_bitwise(stage, sig, want, whole, cut):
    """Pushes of `cut` samples equal the one-push stream, in f32 at 24 kHz and in mu-law at 8 kHz; n samples leave for n that enter;
    blocks and readings do not depend on the cuts."""
    y, z, Ms, As, cg = want[(TARGET, 0)]
    for rate, fmt, k in ((24000, "f32", 0), (8000, "ulaw", 1)):
        stage.set(1, rate, fmt=fmt); stage.set_loudness(1, NORM, TARGET, 0)
        got = run_row(stage, 1, sig, cut)
        if k == 0:
            assert [g.size for g in got[:-1]] == [cut] * (len(got) - 1)
        got = np.concatenate(got)
        assert got.dtype == whole[k].dtype
        np.testing.assert_array_equal(bits(got) if k == 0 else got, bits(whole[k]) if k == 0 else whole[k], err_msg=f"{fmt}, pushes of {cut}")
        assert np.array_equal(bits(stage.loudness_blocks(1)), bits(z))
        check_reading(stage.loudness(1), z, Ms, As, cg)


def test_meter_mode_passes_the_samples(stage, sig, want):
    y, z, Ms, As, cg = want[(TARGET, 0)]
    stage.set(1, 24000); stage.set_loudness(1, METER)
    got = np.concatenate(run_row(stage, 1, sig, 3001))
    assert np.array_equal(bits(got), bits(sig))
    assert np.array_equal(bits(stage.loudness_blocks(1)), bits(z))
    check_reading(stage.loudness(1), z, Ms, As, cg)        # (the gain it would have applied)


def test_off_is_the_stage_without_loudness(stage, sig):
    """A row never set, and one set back to off after it had normalised, return the bits and the counts of a stage that never
    heard of loudness, at 24 kHz f32 (a copy) and at 16 kHz s16; such a row has no reading."""
    for rate, s16 in ((24000, False), (16000, True)):
        fresh = api.PcmStage(0, 1, sig.size)
        fresh.set(0, rate, s16)
        ref = run_row(fresh, 0, sig, 1777)
        fresh.close()
        stage.set(2, rate, s16); stage.set_loudness(2, OFF)      # explicit off on a row that never had the step
        a = run_row(stage, 2, sig, 1777)
        stage.set_loudness(2, NORM, TARGET, 0); stage.push({2: sig[:3000]}); stage.set_loudness(2, OFF)      # ... and after it
        b = run_row(stage, 2, sig, 1777)
        for got in (a, b):
            assert [g.size for g in got] == [r.size for r in ref]
            np.testing.assert_array_equal(np.concatenate(got), np.concatenate(ref))
    with pytest.raises(_lib.Q3Error) as e:
        stage.loudness(2)
    assert e.value.status == Q3_INVALID_ARG
    assert stage.loudness_blocks(2).size == 0


def test_three_rows_against_their_one_row_runs(sig):
    """Rows with different modes, targets, priors and push sizes in the same pushes equal their runs alone."""
    settings = [(NORM, TARGET, 0, 1000), (METER, -1900, 0, 2400), (NORM, -2300, 600, 7001)]
    xs = [sig, sig[::-1].copy(), (sig * f32(0.5))[:N_SIG - 3000]]
    alone = []
    for (mode, target, prior, _), x in zip(settings, xs):
        one = api.PcmStage(0, 1, N_SIG)
        one.set_loudness(0, mode, target, prior)
        alone.append((one.push({0: x}, last=(0,))[0], one.loudness_blocks(0), one.loudness(0)))
        one.close()
    ps = api.PcmStage(0, 3, N_SIG)
    for r, (mode, target, prior, _) in enumerate(settings):
        ps.set_loudness(r, mode, target, prior)
    at = [0, 0, 0]; out = [[], [], []]
    while any(at[r] < xs[r].size for r in range(3)):
        push = {}; last = []
        for r in range(3):
            if at[r] < xs[r].size:
                n = min(settings[r][3], xs[r].size - at[r])
                push[r] = xs[r][at[r]:at[r] + n]; at[r] += n
                if at[r] >= xs[r].size:
                    last.append(r)
        for r, v in ps.push(push, last=last).items():
            out[r].append(v)
    for r in range(3):
        assert np.array_equal(bits(np.concatenate(out[r])), bits(alone[r][0])), r
        assert np.array_equal(bits(ps.loudness_blocks(r)), bits(alone[r][1])) and ps.loudness(r) == alone[r][2], r
    assert np.array_equal(bits(alone[1][0]), bits(xs[1])) and not np.array_equal(bits(alone[0][0]), bits(xs[0]))
    ps.close()


def test_a_nan_moves_no_other_sample_and_no_block(stage, sig):
    x = sig.copy(); z = sig.copy()
    for i in (5000, 5001, 12000):
        x[i] = np.nan if i != 5001 else np.inf; z[i] = 0.0
    stage.set(1, 24000); stage.set_loudness(1, NORM, TARGET, 0)
    a = np.concatenate(run_row(stage, 1, x, 4000)); za = stage.loudness_blocks(1); ra = stage.loudness(1)
    stage.reset(1)
    b = np.concatenate(run_row(stage, 1, z, 4000)); zb = stage.loudness_blocks(1); rb = stage.loudness(1)
    keep = np.ones(sig.size, bool); keep[[5000, 5001, 12000]] = False
    np.testing.assert_array_equal(bits(a[keep]), bits(b[keep]))
    assert np.isnan(a[5000]) and np.isinf(a[5001]) and np.isnan(a[12000])      # the samples themselves leave as they are
    assert np.array_equal(bits(za), bits(zb)) and ra == rb and np.all(np.isfinite(za)) and za.size == 6


def test_digital_silence_keeps_the_prior(stage, sig):
    P = consts_np(TARGET, -600)[1]
    stage.set(1, 24000); stage.set_loudness(1, NORM, TARGET, -600)
    got = np.concatenate(run_row(stage, 1, np.zeros(8 * HOP, f32), 5000))
    r = stage.loudness(1)
    assert np.all(got == 0.0) and r.blocks == 5 and r.gated == 0 and r.mean_square == 0.0 and r.lufs == float("-inf")
    assert bits(f32(r.gain)) == bits(P) and np.all(stage.loudness_blocks(1) == 0.0)
    stage.reset(1)                                          # sound after 0.8 s of silence starts from the prior: its first hop leaves at P,
    x = np.concatenate([np.zeros(8 * HOP, f32), sig[:2 * HOP]])      # the estimate that hop gives ramps in over the next
    got = np.concatenate(run_row(stage, 1, x, 12000))
    assert np.array_equal(bits(got[8 * HOP:9 * HOP]), bits(sig[:HOP] * P))
    assert stage.loudness(1).gated == 2 and not np.array_equal(bits(got[9 * HOP + 1:]), bits(sig[HOP + 1:2 * HOP] * P))


def test_commit_rule(stage, sig, whole, want):
    """A push refused for its cap, and one that lists the row twice, change nothing — samples, blocks, reading —: the next push
    continues bitwise. _set, _reset, _set_tempo, _set_level and _set_loudness keep the setting and restart the row."""
    y, z, Ms, As, cg = want[(TARGET, 0)]
    stage.set(1, 24000); stage.set_tempo(1, 1000); stage.set_level(1, 0, 0); stage.set_loudness(1, NORM, TARGET, 0)
    a = stage.push({1: sig[:11000]})[1]
    assert a.size == 11000
    before = (stage.loudness(1), stage.loudness_blocks(1))
    assert before[0].blocks == 1
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([1], [sig[11000:18000]], [False], cap=[10])
    assert e.value.status == Q3_INVALID_ARG
    with pytest.raises(_lib.Q3Error) as e:
        stage._push_lists([1, 1], [sig[11000:13000], sig[13000:15000]], [False, False])
    assert e.value.status == Q3_INVALID_ARG
    assert stage.loudness(1) == before[0] and np.array_equal(bits(stage.loudness_blocks(1)), bits(before[1]))
    b = stage.push({1: sig[11000:11100]})[1]
    c = stage.push({1: sig[11100:]}, last=(1,))[1]
    np.testing.assert_array_equal(bits(np.concatenate([a, b, c])), bits(whole[0]))
    check_reading(stage.loudness(1), z, Ms, As, cg)
    assert stage.push({1: sig[:0]}, last=(1,))[1].size == 0
    check_reading(stage.loudness(1), z, Ms, As, cg)        # (an empty flush moves nothing)
    for restart in (lambda: stage.reset(1), lambda: stage.set(1, 24000), lambda: stage.set_tempo(1, 1000), lambda: stage.set_level(1, 0, 0),
                    lambda: stage.set_loudness(1, NORM, TARGET, 0)):
        restart()
        stage.push({1: sig[:7000]})
        restart()                                          # in mid-stream
        assert stage.loudness(1).blocks == 0 and stage.loudness_blocks(1).size == 0
        got = np.concatenate(run_row(stage, 1, sig, 12000))
        np.testing.assert_array_equal(bits(got), bits(whole[0]))
    for mode, target, prior in ((3, TARGET, 0), (-1, TARGET, 0), (NORM, -4001, 0), (NORM, -499, 0), (NORM, TARGET, 2401), (METER, TARGET, -6001)):
        with pytest.raises(_lib.Q3Error) as e:
            stage.set_loudness(1, mode, target, prior)
        assert e.value.status == Q3_INVALID_ARG
    stage.reset(1)
    got = np.concatenate(run_row(stage, 1, sig, sig.size))   # the refused settings changed nothing
    np.testing.assert_array_equal(bits(got), bits(whole[0]))


def test_scale_invariance(stage, sig):
    """The same signal at x 2^-2 and x 2^1 with target -1900: powers of two scale every step exactly and neither gain reaches its
    bound, so the outputs are bitwise equal from sample 12000 on (hop 5: both gains are estimates)."""
    outs = []
    for k, scale in enumerate((0.25, 2.0)):
        stage.set(k, 24000); stage.set_loudness(k, NORM, TARGET, 0)
        outs.append(np.concatenate(run_row(stage, k, sig * f32(scale), 4321)))
        r = stage.loudness(k)
        print(f"x {scale}: {r.lufs:.3f} LUFS, gain {r.gain_db:.3f} dB")
        assert -24.0 < r.gain_db < 24.0
    assert abs((stage.loudness(0).lufs + 20 * np.log10(8.0)) - stage.loudness(1).lufs) < 1e-5
    assert np.array_equal(bits(outs[0][12000:]), bits(outs[1][12000:]))
    assert not np.array_equal(bits(outs[0][:12000]), bits(outs[1][:12000]))
    assert np.array_equal(bits(stage.loudness_blocks(0) * f32(64.0)), bits(stage.loudness_blocks(1)))


def test_composition_with_tempo_level_and_rate(stage, sig):
    """tempo 1250 -> loudness (-1400: loud enough for the limiter to have work) -> level (+600, -100) -> 16 kHz s16 in one row,
    streamed, equals the four steps as one-shot stages; the ceiling holds at 24 kHz behind the normaliser."""
    target = -1400
    y = api.resample_gpu(sig, 24000, tempo_permille=1250).samples
    w = api.resample_gpu(y, 24000, target_mb=target).samples
    e = k_energies(y[None, :])[0]
    np.testing.assert_array_equal(bits(w), bits(normalise(y, track(e, target, 0)[2])))
    z = api.resample_gpu(w, 24000, gain_mb=600, ceiling_mb=-100).samples
    g, c = api.pcm_stage_level_coeffs(600, -100)
    print(f"peak behind the normaliser {float(np.max(np.abs(w))):.3f}, x {float(g):.3f} against the ceiling {float(c):.3f}")
    assert float(np.max(np.abs(z))) <= float(c) < float(np.max(np.abs(w * g)))      # max |y| <= c, and the limiter had work
    ref = api.resample_gpu(z, 16000, pcm16=True).samples
    stage.set(3, 16000, True); stage.set_tempo(3, 1250); stage.set_level(3, 600, -100); stage.set_loudness(3, NORM, target, 0)
    for piece in (sig.size, 1920, 333):
        stage.reset(3)
        got = np.concatenate(run_row(stage, 3, sig, piece))
        assert got.dtype == np.int16
        np.testing.assert_array_equal(got, ref, err_msg=f"pieces of {piece}")
    np.testing.assert_array_equal(api.resample_gpu(sig, 16000, pcm16=True, tempo_permille=1250, gain_mb=600, ceiling_mb=-100, target_mb=target).samples, ref)
    stage.set_tempo(3, 1000); stage.set_level(3, 0, 0); stage.set_loudness(3, OFF)


def test_history_bound():
    """4100 hops of noise in pushes of 240 000 samples: 4096 blocks are kept, M is the gate over them, and with M and A frozen every
    later output is mul_rn(x, A_frozen). Block 4095 ends with hop 4098, and hop h ramps from A_(h-2) to A_(h-1): the outputs behind
    the bound are those from hop 4100 on, so two more pushes follow the 4100 hops."""
    rng = np.random.default_rng(9)
    base = (0.05 * rng.standard_normal(240000)).astype(f32)
    T, P, ga, lo, hi = consts_np(TARGET, 0)
    ps = api.PcmStage(0, 1, 240000)
    ps.set_loudness(0, NORM, TARGET, 0)
    for k in range(41):                                    # 4100 hops
        x = base * f32(1.0 + 0.3 * np.sin(0.37 * k))
        out = ps.push({0: x})[0]
        assert out.size == x.size
    r = ps.loudness(0)
    z = ps.loudness_blocks(0)
    assert r.blocks == HIST and z.size == HIST
    M, cg = gate(z, ga)                                    # the gate over 4096 blocks: 64 entries per partial sum
    assert bits(f32(r.mean_square)) == bits(M) and r.gated == cg
    A = min(max(np.sqrt(T / M), lo), hi)
    assert bits(f32(r.gain)) == bits(A) and lo < A < hi
    out = ps.push({0: base[:2 * HOP + 100]})[0]            # hops 4100, 4101 and a part of 4102
    assert np.array_equal(bits(out), bits(base[:2 * HOP + 100] * A))
    out = ps.push({0: base[:HOP] * f32(8.0)}, last=(0,))[0]
    assert np.array_equal(bits(out), bits(base[:HOP] * f32(8.0) * A))
    assert ps.loudness(0) == r and np.array_equal(bits(ps.loudness_blocks(0)), bits(z))
    ps.close()


def test_readings_against_the_fixture():
    """The four signals of the fixture through a metering row: the blocks are the restatement's bit for bit, the integrated
    loudness meets the float64 value within the allowance, api.loudness returns it."""
    g = np.load(GOLDEN)
    ref = reference()
    ps = api.PcmStage(0, 1, max(x[0].size for x in ref.values()))
    ps.set_loudness(0, METER)
    for name in SIGNALS:
        x, e, z, Ms, As, cg = ref[name]
        ps.reset(0)
        out = np.concatenate(run_row(ps, 0, x, 50000))
        assert np.array_equal(bits(out), bits(x))
        assert np.array_equal(bits(ps.loudness_blocks(0)), bits(z)), name
        r = ps.loudness(0)
        check_reading(r, z, Ms, As, cg)
        gap = abs(r.lufs - float(g[name + "_lufs"]))
        print(f"{name}: {r.lufs:.6f} LUFS on the device, {float(g[name + '_lufs']):.6f} in float64: gap {gap:.2e} LU")
        assert gap <= TOL_LU and r.gated == int(g[name + "_gated"])
    ps.close()
    assert abs(api.loudness(ref["sine"][0]) - (-3.01)) <= 0.1
    assert api.loudness(np.zeros(1000, f32)) == float("-inf")
