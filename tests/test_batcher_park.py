"""Parked batcher tickets (DESIGN 4.13, q3_batcher_set_parking / _park / _unpark / _park_info): more requests in flight than rows,
by explicit park / unpark and by the time slice. Every comparison is np.array_equal against a CLOSED ticket with want_pcm = 1 from a
fresh batcher WITHOUT parking (today's code path), computed once per module — never against another parked run. Tiny LM with the
production decoder shape; the requests are those of test_batcher_text (preset, VoiceDesign, x-vector, ICL 5, ICL 20 in rotation)."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from test_batcher_stream import _full_decoder_cfg
from test_batcher_text import _request, _first, _n_init, _cat, _path, LIMITS, OPTS, PATHS

NEW = ["q3_batcher_set_parking", "q3_batcher_park", "q3_batcher_unpark", "q3_batcher_park_info"]
SPF = 1920
Q3_INVALID_ARG, Q3_UNSUPPORTED = 1, 7
SLOTS, STEP, BUDGET, PROMPT = 3, 8, 72, 48
QUEUED, RUNNING, DONE, CANCELLED, PARKED = 0, 1, 2, 4, 5


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_declared_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "q3tts.h")).read()
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
        assert n + "(" in hdr, n
    assert "Q3_TICKET_PARKED = 5" in hdr


def test_null_handles_and_bad_arguments_return_status():
    L = _lib.lib
    i = ctypes.c_int()
    calls = [
        lambda: L.q3_batcher_set_parking(None, 1, 0, 0),
        lambda: L.q3_batcher_park(None, 1),
        lambda: L.q3_batcher_unpark(None, 1),
        lambda: L.q3_batcher_park_info(None, ctypes.byref(i), None, None, None, None, None),
    ]
    for k, f in enumerate(calls):
        assert f() == Q3_INVALID_ARG, k
        assert L.q3_last_error(), k


def test_python_surface():
    for n in ("park", "unpark", "park_info"):
        assert callable(getattr(api.Batcher, n)), n
    assert api.Batcher.PARKED == 5 and q.Batcher.PARKED == 5
    import inspect
    sig = inspect.signature(api.Batcher.__init__).parameters
    assert sig["max_parked"].default == 0 and sig["quantum_frames"].default == 0 and sig["fresh_first"].default is False


# ---------------------------------------------------------------- tiny LM, full decoder, on the GPU
def _batcher(gm, slots=SLOTS, **kw):
    return q.Batcher(gm, slots=slots, frame_budget=BUDGET, prompt_budget=PROMPT, options=q.SynthesisOptions(**OPTS), **kw)


@pytest.fixture(scope="module")
def world():
    """(model, requests, reference, pages in use before any batcher): every request's (codes, PCM) from a closed ticket with
    want_pcm = 1 on a fresh batcher without parking"""
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg(), seed=1234)
    utts = [_request(gm.config, i, L) for i, L in enumerate(LIMITS)]
    pages0 = gm.kv_pool_info()["pages_in_use"]
    b = _batcher(gm)
    want = b.run_all(utts, want_pcm=True, poll_frames=STEP)
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0
    yield gm, utts, want, pages0
    gm.close()


def _status(f):
    try:
        f()
    except _lib.Q3Error as e:
        return e.status
    return 0


def _drain(b, streamed=(), got=None, use_graph=True, max_steps=2000):
    got = {t: [] for t in streamed} if got is None else got
    for _ in range(max_steps):
        running, queued, _f = b.step(STEP, use_graph)
        for t in streamed:
            a, _d = b.read(t)
            if a.size:
                got[t].append(a)
        if running == 0 and queued == 0:
            break
    else:
        raise AssertionError("the batcher did not finish")
    for t in streamed:
        a, done = b.read(t)
        if a.size:
            got[t].append(a)
        assert done, t
    return got


def _check(b, t, want_i, kind, reads=None, state=DONE, n=None):
    assert b.poll(t)[0] == state
    codes, pcm = b.fetch(t)
    n = want_i[0].shape[0] if n is None else n
    np.testing.assert_array_equal(codes, want_i[0][:n])
    if kind == "pcm":
        np.testing.assert_array_equal(pcm, want_i[1][:n * SPF])
    elif kind == "stream":
        np.testing.assert_array_equal(_cat(reads), want_i[1][:n * SPF])


def _policy(limits, slots, max_parked, quantum, step):
    """The header's policy restated for closed tickets without EOS that are all submitted before the first step, FIFO: (parks,
    resumes, moved) of a run driven in steps of `step` frames. Rows are filled from the one waiting list; at the start of every
    piece the time slice parks the row that has run longest since it entered (>= quantum, ties to the lowest row) while something
    waits, no row is free and fewer than max_parked are parked, the head takes the row, and a ticket parked by this round is not
    resumed by it; a piece ends at the step's end, at a row's limit and, while something waits, at a row's quantum."""
    n = len(limits)
    committed, entered, last_row = [0] * n, [0] * n, [-1] * n
    owner, queue, parked, done = [-1] * slots, list(range(n)), [], set()
    c = {"parks": 0, "resumes": 0, "moved": 0}

    def fill():
        for r in range(slots):
            if owner[r] < 0 and queue:
                t = queue.pop(0)
                if t in parked:
                    parked.remove(t); c["resumes"] += 1; c["moved"] += int(r != last_row[t]); entered[t] = committed[t]
                owner[r] = t

    def time_slice():
        mine = []
        while queue and queue[0] not in mine and len(parked) < max_parked and all(o >= 0 for o in owner):
            used = [committed[o] - entered[o] for o in owner]
            if max(used) < quantum:
                return
            r = used.index(max(used)); t = owner[r]
            c["parks"] += 1; parked.append(t); last_row[t] = r; owner[r] = -1; queue.append(t); mine.append(t)
            fill()

    while len(done) < n:
        left = step
        while left > 0:
            fill(); time_slice()
            live = [r for r in range(slots) if owner[r] >= 0]
            piece = left
            for r in live:
                t = owner[r]
                piece = min(piece, limits[t] - committed[t])
                if queue and committed[t] - entered[t] < quantum:
                    piece = min(piece, quantum - (committed[t] - entered[t]))
            if not live:
                break
            for r in live:
                committed[owner[r]] += piece
            left -= piece
            for r in live:
                if committed[owner[r]] == limits[owner[r]]:
                    done.add(owner[r]); owner[r] = -1
        fill()
    return c["parks"], c["resumes"], c["moved"]


@pytest.mark.gpu
@pytest.mark.parametrize("want_kind", ["codes", "pcm", "stream"])
def test_all_kinds_time_sliced(world, want_kind):
    """Twelve requests, limits 5 .. 70, all submitted before the first step; 3 slots, max_parked 8, quantum 4, steps of 8 frames,
    FIFO. On paper: tickets 0-2 enter rows 0-2. Nine fresh tickets wait, and no ticket can end while one of them waits (every
    limit exceeds the quantum, and a row that has used its quantum is parked while the list is not empty), so a fresh ticket only
    enters through a park: at frame 4 tickets 0, 1, 2 are parked (lowest row first) for 3, 4, 5; at frame 8 those for 6, 7, 8; at
    frame 12 tickets 6 and 7 for 9 and 10 — then eight are parked, ticket 8 keeps row 2 and ticket 11 still waits: parks >= 8
    without counting anything later. Ticket 8 (12 frames) ends at frame 20 and ticket 11 takes row 2; ticket 10 (15 frames,
    row 1, from frame 12) ends at frame 27 and the list's head, ticket 0, which left row 0, goes on in row 1: moved >= 1. Every
    ticket finishes, so every park was resumed. The policy reads no clock, so the counts are exact: they are asserted against the
    restatement of the policy above (_policy: 56 parks, 56 resumes, 43 of them into another row)."""
    gm, utts, want, pages0 = world
    expect = _policy(LIMITS, SLOTS, 8, 4, STEP)
    assert expect == (56, 56, 43) and expect[0] >= len(LIMITS)      # every ticket is longer than the quantum and met a waiting list
    b = _batcher(gm, max_parked=8, quantum_frames=4)
    if want_kind == "stream":
        tickets = [b.submit_streamed(u) for u in utts]
    else:
        tickets = [b.submit(u, want_pcm=want_kind == "pcm") for u in utts]
    got = _drain(b, tickets if want_kind == "stream" else ())
    info = b.park_info()
    assert (info["parks"], info["resumes"], info["moved"]) == expect and info["n_parked"] == 0, info
    assert info["max_parked"] == 8 and info["pages_parked"] == 0
    for i, t in enumerate(tickets):
        _check(b, t, want[i], want_kind, got.get(t))
    assert b.stream_info()["blocks_in_use"] == 0
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_waiting_time_in_steps(world, monkeypatch, path):
    """Three tickets of limit 64 fill the rows, a fourth arrives. Today (the control, asserted here): it still waits after the
    next 8-frame step. With quantum 4 and fresh_first it runs in that step, and the ticket it displaced — row 0: all three have
    committed 8 frames, ties go to the lowest row — reads PARKED (max_parked = 1: with room for a second record the slice in the
    middle of the step would park the next ticket and bring this one back already)."""
    gm, utts, _, _ = world
    g = _path(monkeypatch, path)
    four = [_request(gm.config, i, 64) for i in (0, 1, 2, 5)]

    def run(**kw):
        b = _batcher(gm, **kw)
        t = [b.submit(u, want_pcm=True) for u in four[:3]]
        b.step(STEP, g)
        t.append(b.submit(four[3], want_pcm=True))
        b.step(STEP, g)
        states = [b.poll(x)[:2] for x in t]
        _drain(b, use_graph=g)
        out = [b.fetch(x) for x in t]
        b.close()
        return states, out

    s0, ref = run()
    assert s0[3][0] == QUEUED and [s[0] for s in s0[:3]] == [RUNNING] * 3
    s1, got = run(max_parked=1, quantum_frames=4, fresh_first=True)
    assert s1[3][0] == RUNNING and s1[3][1] >= 1
    assert s1[0] == (PARKED, 8)
    for (c, p), (rc, rp) in zip(got, ref):
        assert rc.shape == (64, 16)
        np.testing.assert_array_equal(c, rc); np.testing.assert_array_equal(p, rp)


@pytest.mark.gpu
@pytest.mark.parametrize("fresh_first", [False, True])
def test_waiting_order(world, fresh_first):
    """Two parked tickets that want a row again, then two fresh ones, two free rows: FIFO lets the parked ones in first,
    fresh_first the fresh ones."""
    gm, utts, want, _ = world
    idx = [1, 5, 2, 3]
    b = _batcher(gm, slots=2, max_parked=4, fresh_first=fresh_first)
    A, B = [b.submit(utts[i], want_pcm=True) for i in idx[:2]]
    b.step(4)
    b.park(A); b.park(B)
    assert b.poll(A)[:2] == (PARKED, 4) and b.poll(B)[:2] == (PARKED, 4)
    b.unpark(A); b.unpark(B)
    C, D = [b.submit(utts[i], want_pcm=True) for i in idx[2:]]
    running, queued, _f = b.step(1)
    assert (running, queued) == (2, 2)
    st = [b.poll(t)[0] for t in (A, B, C, D)]
    assert st == ([PARKED, PARKED, RUNNING, RUNNING] if fresh_first else [RUNNING, RUNNING, QUEUED, QUEUED]), st
    _drain(b)
    for i, t in zip(idx, (A, B, C, D)):
        _check(b, t, want[i], "pcm")
    b.close()


@pytest.mark.gpu
def test_explicit_park_and_unpark(world):
    gm, utts, want, pages0 = world
    idx = [1, 4, 7]                                   # 50, 9 and 7 frames
    b = _batcher(gm, max_parked=1)
    t = [b.submit(utts[i], want_pcm=True) for i in idx]
    b.step(4)
    b.park(t[0])
    assert b.poll(t[0])[:2] == (PARKED, 4)
    assert _status(lambda: b.park(t[1])) == Q3_UNSUPPORTED and b.poll(t[1])[0] == RUNNING      # max_parked reached: nothing changes
    info = b.park_info()
    assert info["n_parked"] == 1 and info["parks"] == 1 and info["pages_parked"] >= 1
    for _ in range(4):                                # rows fall free; nobody asked for the parked ticket
        running, queued, _f = b.step(STEP)
    assert (running, queued) == (0, 0) and b.poll(t[0])[:2] == (PARKED, 4)
    assert b.poll(t[1])[0] == DONE and b.poll(t[2])[0] == DONE
    b.park(t[1])                                      # an ended ticket: nothing happens
    b.unpark(t[0])
    running, queued, _f = b.step(1)
    assert running == 1 and b.poll(t[0])[:2] == (RUNNING, 5)
    _drain(b)
    for i, x in zip(idx, t):
        _check(b, x, want[i], "pcm")
    assert b.park_info()["resumes"] == 1
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_open_ticket_is_parked_when_held(world):
    """One row. An open ticket with text for 3 frames runs them and is HELD; a closed ticket waits, so the held row is parked
    (held first) and the closed one runs. Text appended while it is parked is only recorded; it is closed while parked, resumes
    (the closed ticket has used its quantum by then) and both equal their closed references."""
    gm, utts, want, _ = world
    io, ic = 2, 4                                     # x-vector, 20 frames; preset voice, 9 frames
    u = utts[io]; text = list(u.text_ids)
    b = _batcher(gm, slots=1, max_parked=2, quantum_frames=4)
    O = b.submit_open(_first(u, 1), "pcm")
    b.append_text(O, text[1:4])
    C = b.submit(utts[ic], want_pcm=True)
    b.step(STEP)
    assert b.poll(O)[:2] == (PARKED, 3) and b.poll(C)[:2] == (RUNNING, 5)
    b.append_text(O, text[4:9])
    ts = b.text_state(O)
    assert ts["n_text"] == 9 and ts["frames_committed"] == 3 and ts["frames_runnable"] == 5 and not ts["closed"]
    assert b.poll(O)[0] == PARKED
    b.append_text(O, text[9:], last=True)             # parked, then closed
    b.step(STEP)                                      # O is runnable again: C (5 frames >= the quantum) makes room, and later O for C
    assert b.poll(O)[1] > 3 and b.park_info()["resumes"] >= 1
    _drain(b)
    _check(b, O, want[io], "pcm"); _check(b, C, want[ic], "pcm")
    info = b.park_info()
    assert info["resumes"] == info["parks"] >= 2
    b.close()


@pytest.mark.gpu
def test_streamed_ticket_with_its_own_output_moves_slots(world):
    """16 kHz PCM16 through q3_batcher_read_out: the ticket is parked in slot 0 and goes on in slot 1; its stream row and output
    stage row follow it. The bytes equal those of the same ticket without parking."""
    gm, utts, want, _ = world

    def run(park):
        b = _batcher(gm, slots=2, **(dict(max_parked=2) if park else {}))
        S = b.submit_streamed(utts[1], sample_rate=16000, pcm16=True)      # 50 frames
        X = b.submit(utts[7], want_pcm=False)                              # 7 frames, row 1
        got = {S: []}
        b.step(STEP)
        a, _d = b.read(S); got[S].append(a)
        if park:
            b.park(S)
            assert b.poll(S)[:2] == (PARKED, 8)
            Y = b.submit(utts[2], want_pcm=False)                          # takes row 0
            b.step(1)
            assert b.poll(Y)[0] == RUNNING
            b.unpark(S)
            b.step(1)
            assert b.poll(S)[:2] == (RUNNING, 9)
        _drain(b, [S], got)
        if park:
            assert b.park_info()["moved"] == 1
        codes, _p = b.fetch(S)
        assert b.stream_info()["blocks_in_use"] == 0
        b.close()
        return codes, _cat([x for x in got[S] if x.size])

    ref, got = run(False), run(True)
    assert ref[1].dtype == np.int16 and ref[1].size > 0
    np.testing.assert_array_equal(got[0], want[1][0]); np.testing.assert_array_equal(ref[0], want[1][0])
    np.testing.assert_array_equal(got[1], ref[1])


@pytest.mark.gpu
@pytest.mark.parametrize("i,kind", [(1, "pcm"), (3, "pcm"), (5, "stream"), (9, "codes")])
def test_cancel_of_a_parked_ticket(world, i, kind):
    """Codes and PCM (an ICL ticket's too; a streamed ticket's reads) are the first n frames of the full run; the record's pages go
    back; q3_batcher_free frees a ticket that is still parked."""
    gm, utts, want, pages0 = world
    b = _batcher(gm, max_parked=2)
    t = b.submit_streamed(utts[i]) if kind == "stream" else b.submit(utts[i], want_pcm=kind == "pcm")
    other = b.submit(utts[6], want_pcm=False)         # 70 frames: stays parked until the batcher is freed
    b.step(STEP)
    reads = []
    if kind == "stream":
        a, _d = b.read(t); reads.append(a)
    b.step(3)
    b.park(t); b.park(other)
    held = b.park_info()["pages_parked"]
    assert held >= 2 and b.poll(t)[:2] == (PARKED, 11)
    b.cancel(t)
    assert b.park_info()["n_parked"] == 1 and b.park_info()["pages_parked"] < held
    if kind == "stream":
        a, done = b.read(t); reads.append(a)
        assert done
    _check(b, t, want[i], kind, reads, state=CANCELLED, n=11)
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_parked_ticket_keeps_its_claim_under_a_page_limit(world):
    """A pool of four pages, three rows, every request one page at worst. Two tickets run, one is parked: three rows hold a page
    each (the vacated row like any idle row) and the record one. A third request would be the fifth page at worst — it waits, as
    it would if the parked ticket still sat in its row, and is not FAILED by a page shortage in the middle of its prefill. The
    parked ticket needs no admission: it re-enters past the waiting head — the row it enters gives its idle page back, and the
    third request then fits, exactly as it does today beside two running rows. Everything ends with the reference bits."""
    gm, utts, want, pages0 = world
    idx = [1, 5, 2]
    gm.kv_pool_limit(pages0 + 4)
    try:
        b = _batcher(gm, max_parked=2)
        A, B = [b.submit(utts[i], want_pcm=True) for i in idx[:2]]
        b.step(4)
        b.park(A)
        assert gm.kv_pool_info()["pages_in_use"] == pages0 + 4
        C = b.submit(utts[idx[2]], want_pcm=True)
        b.step(4)
        assert b.poll(C)[0] == QUEUED and b.poll(A)[0] == PARKED and b.poll(B)[:2] == (RUNNING, 8)
        b.unpark(A)
        b.step(4)
        assert b.poll(A)[:2] == (RUNNING, 8)
        assert b.poll(C)[0] == RUNNING               # the vacated row's page went back with the resume: three rows, four pages, as today
        _drain(b)
        for i, t in zip(idx, (A, B, C)):
            _check(b, t, want[i], "pcm")
        b.close()
    finally:
        gm.kv_pool_limit(0)
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_resume_into_a_row_an_unclosed_open_ticket_left(world):
    """A closed ticket is parked BEFORE the batcher has open-text state. An open ticket then takes the vacated row (which switches
    the hold path on), runs the three frames its text allows and is cancelled unclosed: the row's text_ready stays at 3. The
    parked ticket — 4 frames committed, a record without text_ready — re-enters that row: it must run as the closed row it is
    (held at frame 4 it would end with frames nobody wrote) and equal its reference."""
    gm, utts, want, pages0 = world
    ia, io = 1, 2
    u = utts[io]; text = list(u.text_ids)
    b = _batcher(gm, slots=1, max_parked=1)
    A = b.submit(utts[ia], want_pcm=True)
    b.step(4)
    b.park(A)
    assert b.poll(A)[:2] == (PARKED, 4)
    O = b.submit_open(_first(u, 1), "pcm")
    b.append_text(O, text[1:4])
    b.step(STEP)
    assert b.poll(O)[:2] == (RUNNING, 3) and b.text_state(O)["frames_runnable"] == 0
    b.cancel(O)
    _check(b, O, want[io], "pcm", state=CANCELLED, n=3)
    b.unpark(A)
    _drain(b)
    _check(b, A, want[ia], "pcm")
    b.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0
