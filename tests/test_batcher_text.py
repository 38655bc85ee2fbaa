"""Open batcher tickets (DESIGN 4.9, q3_batcher_submit_open / _append_text / _text_state / _cancel): a ticket's text arrives in
pieces while it waits or speaks, and a ticket can give its row back. On the tiny LM text_dim = 32 always takes the GEMV
projection, so an open run equals the closed run bit for bit: every comparison here is np.array_equal against a
CLOSED ticket with want_pcm = 1 from a fresh batcher (today's code path), computed once per module — never against an open run."""
import ctypes
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt
from test_batcher_stream import _full_decoder_cfg

NEW = ["q3_batcher_submit_open", "q3_batcher_append_text", "q3_batcher_text_state", "q3_batcher_cancel"]
SPF = 1920
Q3_INVALID_ARG, Q3_UNSUPPORTED = 1, 7
SLOTS, STEP, BUDGET, PROMPT = 3, 8, 72, 48
RUNNING, DONE, CANCELLED = 1, 2, 4


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.lib.q3_abi_version() == 1


def test_null_handles_and_bad_arguments_return_status():
    L = _lib.lib
    i = ctypes.c_int(); t64 = ctypes.c_int64()
    ids = (ctypes.c_uint32 * 2)(1, 2)
    calls = [
        lambda: L.q3_batcher_submit_open(None, None, 0, ctypes.byref(t64)),
        lambda: L.q3_batcher_append_text(None, 1, ids, 2, 0),
        lambda: L.q3_batcher_text_state(None, 1, ctypes.byref(i), None, None, None),
        lambda: L.q3_batcher_cancel(None, 1),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error(), k


def test_python_surface():
    for n in ("submit_open", "append_text", "text_state", "cancel"):
        assert callable(getattr(api.Batcher, n)), n
    assert api.Batcher.CANCELLED == 4 and q.Batcher.CANCELLED == 4


# ---------------------------------------------------------------- tiny LM, full decoder, on the GPU
PATHS = ["aql", "hipgraph", "eager"]
LIMITS = [5, 50, 20, 27, 9, 64, 70, 7, 12, 33, 15, 41]
OPTS = dict(eos_token_id=None, max_length=BUDGET, seed=1)
WANTS = ["codes", "pcm", "stream"]


def _path(monkeypatch, path):
    """frame submission path: own AQL queue (default), hipGraphLaunch (Q3_AQL=0, read per session), eager launches"""
    if path == "hipgraph":
        monkeypatch.setenv("Q3_AQL", "0")
    else:
        monkeypatch.delenv("Q3_AQL", raising=False)
    return path != "eager"


def _request(cfg, i, L):
    """kinds in rotation: preset voice, voice design, x-vector clone, ICL with 5 and with 20 reference frames; 24 + i text
    tokens, so that every ICL request has its n_ref + 1 - n_ref_text initial tokens and something left to feed"""
    rng = np.random.default_rng(300 + i)
    text = synthetic_prompt(24 + i, i)
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


def _n_init(u):
    """the fewest text tokens an open request may carry: one, an ICL request n_ref + 1 - n_ref_text"""
    if u.ref_codes is not None and u.ref_text_ids is not None:
        return max(1, len(u.ref_codes) + 1 - len(u.ref_text_ids))
    return 1


def _first(u, k):
    v = api.Utterance(**{f: getattr(u, f) for f in u.__dataclass_fields__})
    v.text_ids = list(u.text_ids)[:k]
    return v


def _batcher(gm, slots=SLOTS):
    return q.Batcher(gm, slots=slots, frame_budget=BUDGET, prompt_budget=PROMPT, options=q.SynthesisOptions(**OPTS))


@pytest.fixture(scope="module")
def world():
    """(model, requests, reference, pages an idle batcher holds): every request's (codes, PCM) from a CLOSED ticket with
    want_pcm = 1 on a fresh batcher."""
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg(), seed=1234)
    utts = [_request(gm.config, i, L) for i, L in enumerate(LIMITS)]
    pages0 = gm.kv_pool_info()["pages_in_use"]
    b = _batcher(gm)
    want = b.run_all(utts, want_pcm=True, poll_frames=STEP)
    idle_pages = gm.kv_pool_info()["pages_in_use"] - pages0      # a drained batcher: what its idle rows keep
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0
    for (codes, pcm), L in zip(want, LIMITS):
        assert codes.shape == (L, 16) and pcm.shape == (L * SPF,)
    yield gm, utts, want, idle_pages
    gm.close()


def _feeder(b, t, rest, sched):
    """a ticket's feeding schedule as a generator that is advanced once before every step"""
    rest = list(rest)
    if sched == 0:                                   # one token before each step
        while len(rest) > 1:
            b.append_text(t, [rest.pop(0)])
            yield
        b.append_text(t, rest, last=True)
    elif sched == 1:                                 # irregular pieces, an empty one and one that crosses a projection group
        sizes = [1, 3, 0, 11, 2, 0, 5]; k = 0
        while True:
            n = sizes[k % len(sizes)]; k += 1
            piece, rest = rest[:n], rest[n:]
            if not rest:
                b.append_text(t, piece, last=True)
                return
            b.append_text(t, piece)
            yield
    elif sched == 2:                                 # everything plus close right after submit
        b.append_text(t, rest, last=True)
    else:                                            # nothing until the ticket has been RUNNING and held for two steps
        held = 0
        while held < 2:
            yield
            ts = b.text_state(t)
            if b.poll(t)[0] == RUNNING and ts["frames_runnable"] == 0 and not ts["closed"]:
                held += 1
        b.append_text(t, rest, last=True)


def _submit(b, u, i, open_, want):
    """(ticket, feeder or None)"""
    if not open_:
        return (b.submit_streamed(u) if want == "stream" else b.submit(u, want_pcm=want == "pcm")), None
    k = _n_init(u)
    t = b.submit_open(_first(u, k), want)
    return t, _feeder(b, t, list(u.text_ids)[k:], i % 4)


def _cat(parts):
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def _drive(b, feeders, streamed, use_graph=True, step=STEP, max_steps=3000):
    """advance every feeder, step, read the streamed tickets — until nothing runs and nothing waits"""
    got = {t: [] for t in streamed}
    live = dict(feeders)
    for _ in range(max_steps):
        for t in list(live):
            try:
                next(live[t])
            except StopIteration:
                del live[t]
        running, queued, _f = b.step(step, use_graph)
        for t in streamed:
            a, _done = b.read(t)
            if a.size:
                got[t].append(a)
        if running == 0 and queued == 0 and not live:
            break
    else:
        raise AssertionError("the batcher did not finish")
    for t in streamed:
        a, done = b.read(t)
        if a.size:
            got[t].append(a)
        assert done, t
    return got


def _want_of(i):
    return WANTS[(i + i // 3) % 3]


def _run_and_compare(gm, utts, want, b, is_open, use_graph=True):
    tickets, feeders, streamed = [], {}, []
    for i, u in enumerate(utts):
        w = _want_of(i)
        t, f = _submit(b, u, i, is_open(i), w)
        tickets.append(t)
        if f is not None:
            feeders[t] = f
        if w == "stream":
            streamed.append(t)
    got = _drive(b, feeders, streamed, use_graph)
    for i, t in enumerate(tickets):
        assert b.poll(t)[0] == DONE, i
        codes, pcm = b.fetch(t)
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
        w = _want_of(i)
        if w == "stream":
            np.testing.assert_array_equal(_cat(got[t]), want[i][1], err_msg=f"request {i}")
        elif w == "pcm":
            np.testing.assert_array_equal(pcm, want[i][1], err_msg=f"request {i}")
    assert b.stream_info()["blocks_in_use"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_open_equals_closed(world, monkeypatch, path):
    """Twelve requests of every kind, greedy and seeded, submitted open with their minimum text and fed under four schedules;
    codes / PCM / concatenated reads are those of the closed reference."""
    gm, utts, want, _ = world
    use_graph = _path(monkeypatch, path)
    b = _batcher(gm)
    _run_and_compare(gm, utts, want, b, lambda i: True, use_graph)
    b.close()


@pytest.mark.gpu
def test_closed_neighbours_of_held_rows(world):
    """Every second ticket submitted closed: closed tickets running beside held rows have the reference bits."""
    gm, utts, want, _ = world
    b = _batcher(gm)
    _run_and_compare(gm, utts, want, b, lambda i: i % 2 == 0)
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("no_stage", [False, True])
def test_queued_and_staged_appends(world, monkeypatch, no_stage):
    """Four tickets on three slots with graph replay: the fourth waits, and is prefilled ahead on the worker once the frame is
    captured. It gets tokens while queued, again after two steps (staged, unless Q3_BAT_NO_STAGE=1), and after it entered its row."""
    gm, utts, want, _ = world
    if no_stage:
        monkeypatch.setenv("Q3_BAT_NO_STAGE", "1")
    else:
        monkeypatch.delenv("Q3_BAT_NO_STAGE", raising=False)
    b = _batcher(gm)
    idx = [1, 3, 9, 2]                                # 50, 27 (ICL), 33 frames; the fourth: 20 frames, x-vector
    first = [b.submit(utts[i], want_pcm=True) for i in idx[:3]]
    u = utts[idx[3]]; text = list(u.text_ids)
    t = b.submit_open(_first(u, 1), "pcm")
    b.append_text(t, text[1:4])                       # queued
    assert b.text_state(t) == {"n_text": 4, "frames_committed": 0, "frames_runnable": 3, "closed": False}
    b.step(STEP); b.step(STEP)
    assert b.poll(t)[0] == q.Batcher.QUEUED
    b.append_text(t, text[4:13])                      # staged: the side session was prefilled with four tokens
    assert b.text_state(t)["frames_runnable"] == 12
    for _ in range(40):
        b.step(STEP)
        if b.poll(t)[0] == RUNNING:
            break
    assert b.poll(t)[0] == RUNNING
    b.step(STEP)
    assert b.text_state(t)["frames_committed"] == 12 and b.poll(t)[1] == 12      # every token received so far was applied, then held
    b.append_text(t, text[13:], last=True)            # in its row
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    for i, tk in zip(idx, first + [t]):
        codes, pcm = b.fetch(tk)
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
        np.testing.assert_array_equal(pcm, want[i][1], err_msg=f"request {i}")
    b.close()


@pytest.mark.gpu
def test_all_rows_held(world):
    """Three open tickets with their text exhausted: a step replays nothing and moves nothing; one append moves one row, by
    exactly the frames its text allows."""
    gm, utts, want, _ = world
    b = _batcher(gm)
    idx = [1, 5, 6]
    tickets = []
    for i in idx:
        t = b.submit_open(_first(utts[i], 1), "codes")
        b.append_text(t, list(utts[i].text_ids)[1:5])
        tickets.append(t)
    running, queued, _f = b.step(STEP)
    assert (running, queued) == (3, 0)
    before = [(b.poll(t)[1], b.text_state(t)) for t in tickets]
    for n, ts in before:
        assert n == 4 and ts == {"n_text": 5, "frames_committed": 4, "frames_runnable": 0, "closed": False}
    running, queued, finished = b.step(STEP)
    assert (running, queued, finished) == (3, 0, 0)
    assert [(b.poll(t)[1], b.text_state(t)) for t in tickets] == before
    b.append_text(tickets[1], list(utts[idx[1]].text_ids)[5:8])
    assert b.text_state(tickets[1])["frames_runnable"] == 3
    running, queued, _f = b.step(STEP)
    assert running == 3
    assert [b.poll(t)[1] for t in tickets] == [4, 7, 4]
    assert [b.text_state(t)["frames_committed"] for t in tickets] == [4, 7, 4]
    for i, t in zip(idx, tickets):                    # ... and they finish with the reference bits
        b.append_text(t, list(utts[i].text_ids)[8 if t == tickets[1] else 5:], last=True)
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    for i, t in zip(idx, tickets):
        np.testing.assert_array_equal(b.fetch(t)[0], want[i][0], err_msg=f"request {i}")
    b.close()


@pytest.mark.gpu
@pytest.mark.parametrize("slots", [20, 33])
def test_wide_flush(slots):
    """One flush carries tokens of every slot: 20 tokens (two full projection groups and a padded one, rows of many slots in one
    group), then one token each and eleven for one ticket, then a step without text, then the rest. Reference: the same requests
    closed, on a batcher of the same width (33 slots: the wide-GEMM family)."""
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg(), seed=1234)
    utts = [_request(gm.config, i, 10 + (i * 5) % 13) for i in range(slots)]
    b = _batcher(gm, slots); want = b.run_all(utts, want_pcm=True, poll_frames=STEP); b.close()
    b = _batcher(gm, slots)
    tickets, pos, streamed = [], [], []
    for i, u in enumerate(utts):
        w = WANTS[i % 3]
        tickets.append(b.submit_open(_first(u, _n_init(u)), w)); pos.append(_n_init(u))
        if w == "stream":
            streamed.append(tickets[-1])

    def give(i, n, last=False):
        text = list(utts[i].text_ids)
        b.append_text(tickets[i], text[pos[i]:pos[i] + n] if n is not None else text[pos[i]:], last)
        pos[i] += n or 0
    for i in range(slots):
        give(i, 1)
    assert b.step(STEP)[0] == slots
    for i in range(slots):
        give(i, 11 if i == 7 else 1)
    b.step(STEP)
    assert [b.text_state(t)["frames_committed"] for t in tickets] == [1 + STEP if i == 7 else 2 for i in range(slots)]
    b.step(STEP)                                      # nothing arrived: the one row that has text left goes on, the others are held
    assert [b.poll(t)[1] for t in tickets] == [12 if i == 7 else 2 for i in range(slots)]
    assert b.step(STEP)[0] == slots                   # ... and now every row is held
    assert [b.text_state(t)["frames_committed"] for t in tickets] == [12 if i == 7 else 2 for i in range(slots)]
    for i in range(slots):
        give(i, None, last=True)
    got = _drive(b, {}, streamed)
    for i, t in enumerate(tickets):
        codes, pcm = b.fetch(t)
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
        if WANTS[i % 3] != "codes":
            np.testing.assert_array_equal(_cat(got[t]) if t in got else pcm, want[i][1], err_msg=f"request {i}")
    b.close(); gm.close()


@pytest.mark.gpu
def test_eos_on_an_open_ticket(world):
    """A live EOS id ends the ticket while its text is still open; later appends and the close are accepted and change nothing,
    and the slot is refilled."""
    gm, utts, want, _ = world
    text = synthetic_prompt(48, 6)
    free = q.Utterance(text, q.Speaker.Ryan, q.Language.English, seed=15, max_length=40)
    free.options = q.SynthesisOptions(**OPTS)
    s1 = gm.session([free], free.options); s1.prefill(); s1.generate(40); c0 = s1.codes(0)[:, 0]; s1.close()
    f = next(f for f in range(9, 39) if f % STEP and c0[f] not in c0[:f])      # frame f's semantic code appears there first
    eos = q.Utterance(text, q.Speaker.Ryan, q.Language.English, seed=15, max_length=40)
    eos.options = q.SynthesisOptions(eos_token_id=int(c0[f]), max_length=BUDGET, seed=1)
    reqs = [utts[2], eos, utts[3], utts[0]]
    b = _batcher(gm); ref = b.run_all(reqs, want_pcm=True, poll_frames=STEP); b.close()
    assert ref[1][0].shape == (f, 16) and ref[1][1].shape == (f * SPF,)         # ... it did end there
    b = _batcher(gm)
    tickets = [b.submit(reqs[0], True), b.submit_open(_first(eos, 1), "pcm"), b.submit(reqs[2], True), b.submit(reqs[3], True)]
    t = tickets[1]
    b.append_text(t, text[1:])                        # all of it, not closed: the row ends on its EOS with the text open
    for _ in range(20):
        b.step(STEP)
        if b.poll(t)[0] == DONE:
            break
    assert b.poll(t)[:2] == (DONE, f) and not b.text_state(t)["closed"]
    assert b.poll(tickets[3])[0] != q.Batcher.QUEUED  # the fourth request has a row
    b.append_text(t, [1, 2, 3])
    b.append_text(t, [], last=True)
    assert b.poll(t)[:2] == (DONE, f)
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    for i, tk in enumerate(tickets):
        codes, pcm = b.fetch(tk)
        np.testing.assert_array_equal(codes, ref[i][0], err_msg=f"request {i}")
        np.testing.assert_array_equal(pcm, ref[i][1], err_msg=f"request {i}")
    b.close()


@pytest.mark.gpu
def test_refusals(world):
    gm, utts, want, _ = world
    L = _lib.lib
    b = _batcher(gm)
    u = utts[0]; text = list(u.text_ids)

    def refused(f, status):
        with pytest.raises(_lib.Q3Error) as e:
            f()
        assert e.value.status == status, e.value

    t = b.submit_open(_first(u, 1), "pcm")
    closed = b.submit(utts[7], want_pcm=True)
    refused(lambda: b.append_text(closed, [1]), Q3_INVALID_ARG)                 # not submitted open
    refused(lambda: b.append_text(4242, [1]), Q3_INVALID_ARG)                   # unknown ticket
    refused(lambda: b.text_state(4242), Q3_INVALID_ARG)
    refused(lambda: b.cancel(4242), Q3_INVALID_ARG)
    refused(lambda: b.append_text(t, [gm.config.text_vocab]), Q3_INVALID_ARG)   # id >= text_vocab
    refused(lambda: b.submit_open(_first(utts[4], 3), "pcm"), Q3_INVALID_ARG)   # ICL, 20 reference frames: needs 18 target tokens
    refused(lambda: b.submit_open(_first(u, 0), "pcm"), Q3_INVALID_ARG)         # no text token at all
    keep = []; r = api.CRequest(); api.fill_request(r, _first(u, 1), b.options, keep); t64 = ctypes.c_int64()
    for bad in (-1, 3):
        assert L.q3_batcher_submit_open(b._h, ctypes.byref(r), bad, ctypes.byref(t64)) == Q3_INVALID_ARG and L.q3_last_error()
    b.append_text(t, text[1:10])
    b.step(STEP)
    # text past the slot (prompt_budget + 1024 rows): nothing of the call is taken, the ticket goes on and can be closed
    refused(lambda: b.append_text(t, [5] * (PROMPT + 1024)), Q3_UNSUPPORTED)
    assert b.text_state(t)["n_text"] == 10
    b.append_text(t, text[10:], last=True)
    refused(lambda: b.append_text(t, [1]), Q3_INVALID_ARG)                      # after the close
    refused(lambda: b.append_text(t, [], last=True), Q3_INVALID_ARG)
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    codes, pcm = b.fetch(t)
    np.testing.assert_array_equal(codes, want[0][0]); np.testing.assert_array_equal(pcm, want[0][1])
    np.testing.assert_array_equal(b.fetch(closed)[0], want[7][0])
    b.close()


@pytest.mark.gpu
def test_cancel(world):
    """A ticket cancelled while queued, staged, running and held, running streamed mid-utterance with unread samples, and DONE
    (no-op). The running ones keep the frames they committed — codes and samples are a prefix of the reference —, their slot is
    refilled in the following step, the other tickets have the reference bits, and blocks and pages come back.
    Pages: an idle row of a drained batcher keeps one page (tests/test_paged_kv.py), so `pages_in_use` is compared with what
    the never-cancelled reference batcher held when it had drained, and with the figure before the first submit once the
    batcher is closed."""
    gm, utts, want, idle_pages = world
    pages0 = gm.kv_pool_info()["pages_in_use"]
    b = _batcher(gm)
    iA, iB, iC, iD, iE, iF = 5, 1, 6, 2, 3, 9          # 64 (preset), 50 (design), 70, | queue: 20, 27 (ICL), 33
    A = b.submit_open(_first(utts[iA], 1), "stream"); b.append_text(A, list(utts[iA].text_ids)[1:])      # all text, left open
    B = b.submit_open(_first(utts[iB], 1), "pcm"); b.append_text(B, list(utts[iB].text_ids)[1:6])       # five frames, then held
    C = b.submit(utts[iC], want_pcm=True)
    D = b.submit_open(_first(utts[iD], 1), "codes"); b.append_text(D, list(utts[iD].text_ids)[1:3])
    E = b.submit_open(_first(utts[iE], _n_init(utts[iE])), "pcm")
    F = b.submit(utts[iF], want_pcm=True)
    b.step(STEP); b.step(STEP)
    assert b.poll(A)[:2] == (RUNNING, 16) and b.poll(B)[:2] == (RUNNING, 5) and b.text_state(B)["frames_runnable"] == 0
    assert b.poll(D)[0] == b.poll(E)[0] == q.Batcher.QUEUED
    b.cancel(E)                                       # queued behind the head
    b.cancel(D)                                       # the head of the queue: staged on the prefill worker by now
    for t in (D, E):
        assert b.poll(t)[:2] == (CANCELLED, 0)
        codes, pcm = b.fetch(t)
        assert codes.shape == (0, 16) and pcm is None
    b.cancel(B)                                       # running and held
    assert b.poll(B)[:2] == (CANCELLED, 5)
    b.cancel(B)                                       # again: nothing happens
    codes, pcm = b.fetch(B)
    np.testing.assert_array_equal(codes, want[iB][0][:5]); np.testing.assert_array_equal(pcm, want[iB][1][:5 * SPF])
    running, queued, _f = b.step(STEP)                # F enters the freed slot in the following step
    assert (running, queued) == (3, 0) and b.poll(F)[:2] == (RUNNING, STEP)
    assert b.poll(A)[1] == 24                         # streamed, mid-utterance, three steps' samples and none of them read
    b.cancel(A)
    assert b.poll(A)[:2] == (CANCELLED, 24)
    parts = []
    while True:
        a, done = b.read(A, 10000)
        parts.append(a)
        if done:
            break
        assert a.size
    np.testing.assert_array_equal(_cat(parts), want[iA][1][:24 * SPF])
    codes, none = b.fetch(A)
    assert none is None
    np.testing.assert_array_equal(codes, want[iA][0][:24])
    while True:
        running, queued, _f = b.step(STEP)
        if running == 0 and queued == 0:
            break
    assert b.poll(F)[0] == DONE
    b.cancel(F)                                       # DONE: a no-op
    assert b.poll(F)[0] == DONE
    for i, t in ((iC, C), (iF, F)):
        codes, pcm = b.fetch(t)
        np.testing.assert_array_equal(codes, want[i][0], err_msg=f"request {i}")
        np.testing.assert_array_equal(pcm, want[i][1], err_msg=f"request {i}")
    assert b.stream_info()["blocks_in_use"] == 0
    assert gm.kv_pool_info()["pages_in_use"] - pages0 == idle_pages
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0


# ---------------------------------------------------------------- 1.7B (synthetic weights)
@pytest.mark.gpu
def test_1_7b_open_tickets_match_fixture():
    """The benchmark's eight 512-token prompts (tests/golden/bench_1_7b_codes.npz) through a 4-slot batcher as open tickets,
    opened with a few tokens and fed in irregular pieces across steps, greedy, max_length 24: the codes of all eight equal the
    fixture's first 24 frames. No tolerance (DESIGN 4.10 reports no divergence for this input at session level)."""
    from qwen3_tts_rs_amd import synth
    from make_golden_bench import bench_utt
    L, B = 24, 8
    ref = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_1_7b_codes.npz"))["greedy_codes"]
    gm = q.Qwen3TTS.from_synthetic(q.qwen3_tts_1_7b(), seed=synth.DEFAULT_SEED)
    opts = q.SynthesisOptions(max_length=L, eos_token_id=None, seed=42, temperature=0.0)
    b = q.Batcher(gm, slots=4, frame_budget=L, prompt_budget=16, options=opts)
    utts = [bench_utt(i) for i in range(B)]
    pos = [1 + (3 * i) % 5 for i in range(B)]
    tickets = [b.submit_open(_first(u, pos[i]), "codes") for i, u in enumerate(utts)]
    held = 0
    for it in range(40 * L):
        for i in range(B):
            k = (it * 7 + i * 3) % 5 if (it + i) % 3 else 0             # 0 .. 4 tokens, some steps none
            text = list(utts[i].text_ids)
            if k and pos[i] < len(text) and b.poll(tickets[i])[0] in (q.Batcher.QUEUED, RUNNING):
                b.append_text(tickets[i], text[pos[i]:pos[i] + k]); pos[i] += k
        running, queued, _f = b.step(3)
        held += sum(1 for t in tickets if b.poll(t)[0] == RUNNING and b.text_state(t)["frames_runnable"] == 0)
        if running == 0 and queued == 0:
            break
    assert held > 0                                                     # rows really waited for text
    for i, t in enumerate(tickets):
        codes, _ = b.fetch(t)
        np.testing.assert_array_equal(codes, ref[i][:L], err_msg=f"request {i}")
    b.close(); gm.close()
