"""Streamed batcher tickets (DESIGN 4.9, q3_batcher_submit_streamed / _read / _stream_info): a ticket's audio is delivered while
it runs, through a block-allocated codec stream with one stream row per slot. The concatenation of everything `read` returns
for a ticket is the PCM the same request gives with want_pcm = 1 on a fresh batcher, and its codes are the same — the same BITS
(np.array_equal; no tolerance anywhere in this file). Tiny LM with the production decoder shape, seeded options."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import manifest_handle, synthetic_prompt

NEW = ["q3_batcher_submit_streamed", "q3_batcher_read", "q3_batcher_stream_info"]
SPF = 1920
Q3_INVALID_ARG, Q3_OOM = 1, 8
SLOTS, STEP, BUDGET, PROMPT = 3, 7, 70, 48


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    for n in ("submit_streamed", "read", "stream_info"):
        assert callable(getattr(api.Batcher, n)), n
    assert callable(api.Qwen3TTS.synthesize_continuous_streaming)


def test_no_device_no_fallback():
    """Null handles get a status and a message from every new entry point. A manifest-only model (device -1) never gets as far
    as a streamed ticket: no batcher can be opened on it."""
    L = _lib.lib
    i = ctypes.c_int(); sz = ctypes.c_size_t(); t64 = ctypes.c_int64(); b = ctypes.c_void_p()
    h = manifest_handle(q.tiny())
    assert L.q3_batcher_create(h, 2, 16, 0, ctypes.byref(b)) != 0
    assert L.q3_last_error() and not b.value
    L.q3_model_free(h)
    calls = [
        lambda: L.q3_batcher_submit_streamed(None, None, ctypes.byref(t64)),
        lambda: L.q3_batcher_read(None, 1, None, 0, ctypes.byref(sz), ctypes.byref(i)),
        lambda: L.q3_batcher_stream_info(None, ctypes.byref(i), ctypes.byref(sz), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error(), k


# ---------------------------------------------------------------- GPU
def _full_decoder_cfg():
    t = q.tiny()
    return q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads,
                      n_kv_heads=t.n_kv_heads, cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers,
                      cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads, name="tiny-lm-full-decoder")


# twelve requests: max_length 5 .. 70 in an order that gives each of the three slots four tickets (a ticket enters the slot
# that frees first: _schedule below), kinds in rotation: preset voice, voice design, x-vector clone, ICL with 5 and 20
# reference frames
LIMITS = [5, 50, 20, 27, 9, 64, 70, 7, 12, 33, 15, 41]
OPTS = dict(eos_token_id=None, max_length=BUDGET, seed=1)


def _request(cfg, i, L):
    rng = np.random.default_rng(300 + i)
    text = synthetic_prompt(5 + i, i)
    kind = i % 5
    if kind == 0:
        u = q.Utterance(text, q.Speaker.Ryan, q.Language.English)
    elif kind == 1:
        u = q.Utterance(text, language=q.Language.German, instruct_ids=synthetic_prompt(7, 50 + i))
    else:
        xv = rng.standard_normal(cfg.hidden).astype(np.float32)
        if kind == 2:
            u = q.Utterance(text, language=q.Language.French, xvector=xv)
        else:
            n_ref = 5 if kind == 3 else 20
            ref = rng.integers(0, 2048, size=(n_ref, 16)).astype(np.uint32)
            u = q.Utterance(text, language=q.Language.French, xvector=xv, ref_codes=ref, ref_text_ids=synthetic_prompt(3, 90 + i))
    u.seed = 700 + i; u.max_length = L
    u.options = q.SynthesisOptions(temperature=0.0 if i % 3 == 0 else 0.9, **OPTS)
    return u


def _schedule(lengths, slots=SLOTS):
    """the batcher's placement without EOS: FIFO, a ticket enters the free slot of lowest index at the frame a slot frees.
    Returns (tickets served per slot, frames until the last row ends, the frame at which each ticket enters its slot)."""
    free = [0] * slots; served = [0] * slots; starts = []
    for n in lengths:
        s = free.index(min(free)); starts.append(free[s]); free[s] += n; served[s] += 1
    return served, max(free), starts


def _batcher(gm):
    return q.Batcher(gm, slots=SLOTS, frame_budget=BUDGET, prompt_budget=PROMPT, options=q.SynthesisOptions(**OPTS))


@pytest.fixture(scope="module")
def world():
    """(model, requests, reference): every request's (codes, PCM) with want_pcm = 1 from a fresh batcher, computed once."""
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg(), seed=1234)
    utts = [_request(gm.config, i, L) for i, L in enumerate(LIMITS)]
    b = _batcher(gm)
    want = b.run_all(utts, want_pcm=True, poll_frames=STEP)
    b.close()
    for (codes, pcm), L in zip(want, LIMITS):
        assert codes.shape == (L, 16) and pcm.shape == (L * SPF,)
    yield gm, utts, want
    gm.close()


def _drive(b, tickets, streamed, cap=None, read=True, step=STEP, entered=None):
    """step until nothing runs and nothing waits; after every step read each streamed ticket (all that landed, or pieces of at
    most `cap` samples). Returns (pieces per ticket, steps taken). entered (a dict) receives, for every ticket that a poll after
    a step finds in the middle of its run, the frame of the batcher's clock at which it entered its row."""
    got = {t: [] for t in tickets if streamed[t]}
    open_ = set(got)
    limits = dict(zip(tickets, LIMITS))             # (entered: the tickets are the twelve requests in order)

    def drain():
        for t in sorted(open_):
            while True:
                a, done = b.read(t, cap)
                if a.size:
                    got[t].append(a)
                if done:
                    open_.discard(t)
                if done or a.size == 0 or cap is None:
                    break
    steps = 0
    for _ in range(400):
        running, queued, _f = b.step(step)
        steps += 1
        if entered is not None:
            for t in tickets:
                st, n, _ns = b.poll(t)
                if t not in entered and st == q.Batcher.RUNNING and 0 < n < limits[t]:
                    entered[t] = steps * step - n
        if read:
            drain()
        if running == 0 and queued == 0:
            break
    else:
        raise AssertionError("the batcher did not finish")
    drain()
    assert not open_
    return got, steps


def _cat(parts):
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


@pytest.mark.gpu
def test_twelve_streamed_tickets_three_slots(world):
    gm, utts, want = world
    served, makespan, starts = _schedule(LIMITS)
    assert min(served) >= 4, served                  # every slot is reused at least three times ...
    b = _batcher(gm)
    tickets = [b.submit_streamed(u) for u in utts]
    entered = {}
    got, steps = _drive(b, tickets, {t: True for t in tickets}, entered=entered)
    # ... and that is what the batcher did: every ticket that a poll caught inside its run (all but the 5-frame one, which
    # starts and ends inside one step) entered its row at the frame _schedule says, i.e. when the slot it names became free
    assert steps == -(-makespan // STEP)
    assert len(entered) >= 11, sorted(entered)
    for i, t in enumerate(tickets):
        if t in entered:
            assert entered[t] == starts[i], (i, entered[t], starts[i])
    info = b.stream_info()
    assert info["block_frames"] == 128 and 0 < info["blocks_peak"] <= SLOTS and info["blocks_total"] <= SLOTS
    cs = gm.codec_stream(1, 8, block_frames=128)
    assert info["block_bytes"] == cs.info()["block_bytes"] > 0      # the stream's own figure
    cs.close()
    for i, t in enumerate(tickets):
        assert b.poll(t)[0] == q.Batcher.DONE
        np.testing.assert_array_equal(_cat(got[t]), want[i][1], err_msg=f"request {i}")
        codes, pcm = b.fetch(t)
        assert pcm is None
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
    assert b.stream_info()["blocks_in_use"] == 0     # every ticket finished and fetched: no row holds a block
    b.close()


@pytest.mark.gpu
def test_every_second_ticket_not_streamed(world):
    gm, utts, want = world
    b = _batcher(gm)
    tickets = [b.submit_streamed(u) if i % 2 == 0 else b.submit(u, want_pcm=True) for i, u in enumerate(utts)]
    streamed = {t: i % 2 == 0 for i, t in enumerate(tickets)}
    got, _ = _drive(b, tickets, streamed)
    for i, t in enumerate(tickets):
        codes, pcm = b.fetch(t)
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
        np.testing.assert_array_equal(_cat(got[t]) if streamed[t] else pcm, want[i][1], err_msg=f"request {i}")
    assert b.stream_info()["blocks_in_use"] == 0
    b.close()


@pytest.mark.gpu
def test_reads(world):
    """Pieces of at most 1000 samples are consecutive and complete; nothing before the first step; done comes exactly with the
    last sample; an unknown ticket and a non-streamed one get a status."""
    gm, utts, want = world
    b = _batcher(gm)
    tickets = [b.submit_streamed(u) for u in utts[:4]]
    plain = b.submit(utts[4], want_pcm=True)
    a, done = b.read(tickets[0], 1000)
    assert a.size == 0 and not done
    for bad in (plain, 12345):
        with pytest.raises(_lib.Q3Error) as e:
            b.read(bad, 1000)
        assert e.value.status == Q3_INVALID_ARG
    streamed = {t: True for t in tickets}; streamed[plain] = False
    got, _ = _drive(b, tickets + [plain], streamed, cap=1000)
    for i, t in enumerate(tickets):
        total = LIMITS[i] * SPF
        sizes = [p.size for p in got[t]]
        assert all(0 < s <= 1000 for s in sizes) and sum(sizes) == total, (i, sizes[-3:])
        np.testing.assert_array_equal(_cat(got[t]), want[i][1], err_msg=f"request {i}")
    # done exactly with the last sample: a finished ticket read up to its last sample but one is not done
    t = b.submit_streamed(utts[0])
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    total = LIMITS[0] * SPF
    a, done = b.read(t, total - 1)
    assert a.size == total - 1 and not done
    z, done0 = b.read(t, 0)
    assert z.size == 0 and not done0
    last, done = b.read(t, 1000)
    assert last.size == 1 and done
    np.testing.assert_array_equal(np.concatenate([a, last]), want[0][1])
    a, done = b.read(t, 1000)
    assert a.size == 0 and done
    b.close()


@pytest.mark.gpu
def test_steps_back_to_back_then_read(world):
    """No read until every ticket has finished: the jobs queue up behind the steps and nothing is lost."""
    gm, utts, want = world
    b = _batcher(gm)
    idx = [1, 3, 4, 0, 2, 8]
    tickets = [b.submit_streamed(utts[i]) for i in idx]
    got, _ = _drive(b, tickets, {t: True for t in tickets}, read=False)
    for i, t in zip(idx, tickets):
        np.testing.assert_array_equal(_cat(got[t]), want[i][1], err_msg=f"request {i}")
    b.close()


@pytest.mark.gpu
def test_fetch_of_a_streamed_ticket(world):
    gm, utts, want = world
    b = _batcher(gm)
    t = b.submit_streamed(utts[3]); other = b.submit_streamed(utts[2])
    b.step(STEP)
    with pytest.raises(_lib.Q3Error, match="has not finished"):
        b.fetch(t)
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    n = LIMITS[3]
    codes = np.zeros((n, 16), np.uint32); pcm = np.zeros(n * SPF, np.float32)
    st = _lib.lib.q3_batcher_fetch(b._h, t, codes.ctypes.data_as(ctypes.c_void_p), n, pcm.ctypes.data_as(ctypes.c_void_p), pcm.size)
    assert st == Q3_INVALID_ARG and b"q3_batcher_read" in _lib.lib.q3_last_error()
    assert b.poll(t)[0] == q.Batcher.DONE            # refused, not released
    codes, none = b.fetch(t)                         # unread samples are dropped
    assert none is None
    np.testing.assert_array_equal(codes, want[3][0])
    for f in (lambda: b.poll(t), lambda: b.read(t, 10), lambda: b.fetch(t)):
        with pytest.raises(_lib.Q3Error, match="unknown ticket"):
            f()
    a, done = b.read(other)                          # the neighbour is untouched
    assert done
    np.testing.assert_array_equal(a, want[2][1])
    b.close()


@pytest.mark.gpu
def test_block_limit_fails_the_long_ticket_alone(world, monkeypatch):
    """Blocks of 32 frames, four of them at most (Q3_BAT_STREAM_BLOCK_FRAMES / Q3_BAT_STREAM_MAX_BLOCKS, read when the batcher is
    created). The 70-frame ticket needs a third block at its frame 65 while two short tickets (one block each, the queue keeps
    both other slots busy past that frame) hold the rest: that push is refused, the long ticket alone ends FAILED with the
    pool's message, and every short ticket has its bits."""
    gm, utts, want = world
    monkeypatch.setenv("Q3_BAT_STREAM_BLOCK_FRAMES", "32")
    monkeypatch.setenv("Q3_BAT_STREAM_MAX_BLOCKS", "4")
    b = _batcher(gm)
    long_i, short_i = 6, [2, 3, 10, 8, 0, 7, 4, 11, 1]            # 70 | 20 27 15 12 5 7 9 41 50 (27 and 12: ICL, 5 reference frames)
    assert LIMITS[long_i] == 70
    tickets = [b.submit_streamed(utts[i]) for i in [long_i] + short_i]
    got, _ = _drive(b, tickets[1:], {t: True for t in tickets[1:]}, step=5)
    assert b.poll(tickets[0])[0] == q.Batcher.FAILED
    with pytest.raises(_lib.Q3Error, match="block pool exhausted") as e:
        b.read(tickets[0], 1000)
    assert e.value.status == Q3_OOM
    with pytest.raises(_lib.Q3Error, match="block pool exhausted"):
        b.fetch(tickets[0])
    for i, t in zip(short_i, tickets[1:]):
        np.testing.assert_array_equal(_cat(got[t]), want[i][1], err_msg=f"request {i}")
        np.testing.assert_array_equal(b.fetch(t)[0], want[i][0], err_msg=f"request {i}")
    info = b.stream_info()
    assert info["block_frames"] == 32 and info["blocks_in_use"] == 0 and info["blocks_peak"] <= 4
    b.close()


@pytest.mark.gpu
def test_row_that_ends_on_eos_inside_a_step(world):
    """A live EOS id: the streamed row ends inside a step, between two hand-overs. Only the frames up to its end are vocoded —
    the reads are the want_pcm PCM of the same request, no sample more — and the neighbours keep their bits."""
    gm, utts, want = world
    free = q.Utterance(synthetic_prompt(10, 6), q.Speaker.Ryan, q.Language.English, seed=15, max_length=40)
    free.options = q.SynthesisOptions(**OPTS)
    s1 = gm.session([free], free.options); s1.prefill(); s1.generate(40); c0 = s1.codes(0)[:, 0]; s1.close()
    f = next(f for f in range(9, 39) if f % STEP and c0[f] not in c0[:f])      # frame f's semantic code appears there first
    eos = q.Utterance(synthetic_prompt(10, 6), q.Speaker.Ryan, q.Language.English, seed=15, max_length=40)
    eos.options = q.SynthesisOptions(eos_token_id=int(c0[f]), max_length=BUDGET, seed=1)
    reqs = [utts[2], eos, utts[3], utts[0]]
    b = _batcher(gm); ref = b.run_all(reqs, want_pcm=True, poll_frames=STEP); b.close()
    assert ref[1][0].shape == (f, 16) and ref[1][1].shape == (f * SPF,)         # ... it did end there
    b = _batcher(gm)
    tickets = [b.submit_streamed(u) for u in reqs]
    got, _ = _drive(b, tickets, {t: True for t in tickets})
    for i, t in enumerate(tickets):
        np.testing.assert_array_equal(_cat(got[t]), ref[i][1], err_msg=f"request {i}")
        np.testing.assert_array_equal(b.fetch(t)[0], ref[i][0], err_msg=f"request {i}")
    assert b.stream_info()["blocks_in_use"] == 0
    b.close()


@pytest.mark.gpu
def test_synthesize_continuous_streaming(world):
    gm, utts, want = world
    pieces = {i: [] for i in range(5)}; ends = []

    def on_audio(i, samples, done):
        assert i not in ends
        pieces[i].append(samples)
        if done:
            ends.append(i)
    codes = gm.synthesize_continuous_streaming(utts[:5], q.SynthesisOptions(**OPTS), slots=2, poll_frames=STEP, on_audio=on_audio)
    assert sorted(ends) == list(range(5))
    for i in range(5):
        np.testing.assert_array_equal(codes[i], want[i][0], err_msg=f"request {i}")
        np.testing.assert_array_equal(_cat(pieces[i]), want[i][1], err_msg=f"request {i}")
