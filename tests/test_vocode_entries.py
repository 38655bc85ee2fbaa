"""Every entry that turns a row's frames into samples goes through ONE range decode (vocode_enqueue, q3_codec_run.hip): the entries
must hand out the same BITS for the same frames (-m gpu; np.testing.assert_array_equal on float32 PCM, no tolerance).

Tiny synthetic model, max_length 40, chunk 10: a row's third chunk starts at frame 20 > CODEC_CTX_FRAMES = 12, so the convolutional
stack starts at frame 0 for some chunks and segments and past it for others.

  * three CustomVoice rows with EOS on (the sampler of test_decode_resident._opts(True)). Under synthetic weights that sampler
    never draws EOS before frame 40, so rows 1 and 2 carry limits of their own (27 and 33) and the rows do end at different frames:
    run() serial, overlapped and as a one-row session (the one-lane fallback), decode(b), decode(b, f0, f1) pieces against
    decode_codes of the same slice, the chunks of stream mode 1, and a batcher ticket;
  * one ICL row (the one of test_ragged_batch): decode(0), run(), a batcher ticket, a parked ticket's cancel, and
    decode_codes([ref ; codes])[n_ref * 1920:] — which pins the cut at n_ref * samples_per_frame independently of the session;
  * the refusals: a short buffer refuses q3_session_run (serial path) before any sample lands in any row, and q3_session_decode
    says "pcm buffer too small"."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from common import synthetic_prompt
from test_ragged_batch import _mixed

pytestmark = pytest.mark.gpu

SPF, CHUNK, FRAMES, CTX = 1920, 10, 40, 12
LIMITS = [40, 27, 33]                         # rows that end at different frames, none on a chunk boundary but the first
SERIAL = {"Q3_DECODE_OVERLAP": "0"}
OVERLAPPED = {"Q3_DECODE_OVERLAP": "1", "Q3_DECODE_SEG": "16", "Q3_DECODE_TAIL": "16"}
PARKED, CANCELLED, DONE = 5, 4, 2


def _opts(eos=True):
    if eos:
        return q.SynthesisOptions(max_length=FRAMES, temperature=1.3, top_k=0, top_p=1.0, seed=11, min_new_tokens=2, chunk_frames=CHUNK)
    return q.SynthesisOptions(max_length=FRAMES, seed=11, eos_token_id=None, chunk_frames=CHUNK)


def _utts():
    return [q.Utterance(synthetic_prompt(4 + i, i), q.Speaker.Ryan, q.Language.English, seed=42 + i, max_length=LIMITS[i]) for i in range(3)]


def _run(gm, utts, opts, env):
    """(samples per row, codes per row) of Session.run() under `env`"""
    with pytest.MonkeyPatch.context() as mp:
        for k in ("Q3_DECODE_OVERLAP", "Q3_DECODE_SEG", "Q3_DECODE_TAIL", "Q3_DECODE_RESIDENT", "Q3_DECODE_LOG"):
            mp.delenv(k, raising=False)
        for k, v in env.items():
            mp.setenv(k, v)
        s = gm.session(utts, opts)
        audio, timing = s.run()
        codes = [s.codes(b).copy() for b in range(len(utts))]
        s.close()
    assert timing.generation_frames == sum(len(c) for c in codes)
    return [a.samples for a in audio], codes


@pytest.fixture(scope="module")
def gm():
    m = q.Qwen3TTS.from_synthetic(q.tiny(), seed=1234)
    yield m
    m.close()


@pytest.fixture(scope="module")
def rows(gm):
    """(codes, PCM) of every CustomVoice row from the serial run(), computed once and never written to"""
    pcm, codes = _run(gm, _utts(), _opts(), SERIAL)
    lens = [len(c) for c in codes]
    print("frames per row:", lens)
    assert max(lens) > CHUNK + CTX, lens          # a chunk and a segment whose stack starts past frame 0 exist
    assert len(set(lens)) == 3 and all(n <= L for n, L in zip(lens, LIMITS)), lens
    for b in range(3):
        assert pcm[b].shape == (lens[b] * SPF,) and np.isfinite(pcm[b]).all() and np.abs(pcm[b]).max() > 0
        pcm[b].setflags(write=False); codes[b].setflags(write=False)
    return codes, pcm


def test_run_overlapped_and_default(gm, rows):
    codes, pcm = rows
    for env in (OVERLAPPED, {}):                  # {}: Q3_DECODE_OVERLAP unset, the default of a session of three rows
        got, got_codes = _run(gm, _utts(), _opts(), env)
        for b in range(3):
            np.testing.assert_array_equal(got_codes[b], codes[b])
            np.testing.assert_array_equal(got[b], pcm[b], err_msg=f"{env} row {b}")


def test_run_one_lane(gm, rows):
    """a one-row session takes run()'s one-lane fallback (Q3_DECODE_PAIRS is read once per process and stays unset)"""
    codes, pcm = rows
    for b, u in enumerate(_utts()):
        got, got_codes = _run(gm, [u], _opts(), SERIAL)
        np.testing.assert_array_equal(got_codes[0], codes[b])
        np.testing.assert_array_equal(got[0], pcm[b], err_msg=f"row {b}")


def test_decode_whole_pieces_and_chunks(gm, rows):
    codes, pcm = rows
    s = gm.session(_utts(), _opts())
    _lib.check(_lib.lib.q3_session_set_stream_mode(s._h, 1))
    s.prefill(); s.generate(FRAMES)
    for b in range(3):
        n = len(codes[b])
        np.testing.assert_array_equal(s.codes(b), codes[b])
        np.testing.assert_array_equal(s.decode(b), pcm[b], err_msg=f"decode({b})")
        # a piece is an utterance of its own: q3_decode_codes of the same slice
        for f0, f1 in {(0, min(7, n)), (min(3, n - 1), n), (n // 2, n // 2 + 1), (max(n - CTX - 1, 0), n)}:
            np.testing.assert_array_equal(s.decode(b, f0, f1), gm.decode_codes(codes[b][f0:f1]).samples, err_msg=f"decode({b}, {f0}, {f1})")
        assert s.decode(b, n, n).size == 0
    # stream mode 1: the chunks of a row concatenate to its whole decode
    for b in range(3):
        parts, done = [], False
        for _ in range(FRAMES // CHUNK + 1):
            a, done = s.next_chunk_row(b)
            if a is not None:
                assert len(a) % SPF == 0 and len(a) <= CHUNK * SPF
                parts.append(a.samples)
            if done:
                break
        assert done
        np.testing.assert_array_equal(np.concatenate(parts), pcm[b], err_msg=f"chunks of row {b}")
    s.close()


def test_batcher_ticket(gm, rows):
    codes, pcm = rows
    b = q.Batcher(gm, slots=3, frame_budget=FRAMES, prompt_budget=32, options=_opts())
    got = b.run_all(_utts(), want_pcm=True, poll_frames=8)
    b.close()
    for r in range(3):
        np.testing.assert_array_equal(got[r][0], codes[r])
        np.testing.assert_array_equal(got[r][1], pcm[r], err_msg=f"ticket of row {r}")


# ---------------------------------------------------------------- one ICL row
def _icl(gm):
    u = _mixed(gm.config)[4]
    assert u.ref_codes is not None and u.ref_text_ids is not None
    return u, q.SynthesisOptions(max_length=20, eos_token_id=None, seed=1)


def test_icl_entries(gm):
    u, host = _icl(gm)
    ref = np.asarray(u.ref_codes, np.uint32).reshape(-1, 16)
    n_ref = ref.shape[0]
    s = gm.session([u], host)
    s.prefill(); s.generate(20)
    codes, full = s.codes(0).copy(), s.decode(0).copy()
    s.close()
    n = codes.shape[0]
    assert n == u.max_length and full.shape == (n * SPF,)
    # the cut is n_ref * samples_per_frame: the whole-utterance decode of [ref ; codes] without the reference frames' samples
    np.testing.assert_array_equal(full, gm.decode_codes(np.concatenate([ref, codes])).samples[n_ref * SPF:])
    got, got_codes = _run(gm, [u], host, {})
    np.testing.assert_array_equal(got_codes[0], codes)
    np.testing.assert_array_equal(got[0], full, err_msg="run()")
    b = q.Batcher(gm, slots=1, frame_budget=FRAMES, prompt_budget=48, options=host, max_parked=1)
    bc, bp = b.run_all([u], want_pcm=True, poll_frames=8)[0]
    np.testing.assert_array_equal(bc, codes)
    np.testing.assert_array_equal(bp, full, err_msg="ticket")
    # a parked ticket's cancel decodes the frames it has committed from the host copy of the codes
    t = b.submit(u, want_pcm=True)
    b.step(4)
    b.park(t)
    st, k, _ns = b.poll(t)
    assert st == PARKED and 0 < k < n
    b.cancel(t)
    assert b.poll(t)[0] == CANCELLED
    cc, cp = b.fetch(t)
    b.close()
    np.testing.assert_array_equal(cc, codes[:k])
    s = gm.session([u], host)
    s.prefill(); s.generate(k)
    part = s.decode(0, 0, k) if s.frames(0)[0] == k else None
    s.close()
    assert part is not None and part.shape == (k * SPF,)
    np.testing.assert_array_equal(cp, part, err_msg="cancel of the parked ticket")
    np.testing.assert_array_equal(cp, gm.decode_codes(np.concatenate([ref, codes[:k]])).samples[n_ref * SPF:])


# ---------------------------------------------------------------- refusals
def test_short_buffer_refuses_run_before_any_sample(gm, monkeypatch):
    monkeypatch.setenv("Q3_DECODE_OVERLAP", "0")
    s = gm.session(_utts(), _opts(eos=False))
    caps = [LIMITS[0] * SPF, LIMITS[1] * SPF - 1, LIMITS[2] * SPF]
    bufs = [np.full(FRAMES * SPF, np.nan, np.float32) for _ in range(3)]
    ptrs = (ctypes.c_void_p * 3)(*[x.ctypes.data_as(ctypes.c_void_p) for x in bufs])
    ns = (ctypes.c_size_t * 3)()
    with pytest.raises(_lib.Q3Error, match="pcm buffer too small"):
        _lib.check(_lib.lib.q3_session_run(s._h, 1, ptrs, (ctypes.c_size_t * 3)(*caps), ns, None))
    assert [s.frames(b)[0] for b in range(3)] == LIMITS
    for b in range(3):
        assert np.isnan(bufs[b]).all(), b
    s.close()


def test_short_buffer_refuses_decode(gm):
    s = gm.session(_utts()[:1], _opts(eos=False))
    s.prefill(); s.generate(CHUNK)
    out = np.full(CHUNK * SPF, np.nan, np.float32)
    got = ctypes.c_size_t()
    for f0, f1 in ((0, CHUNK), (2, CHUNK)):
        with pytest.raises(_lib.Q3Error, match="pcm buffer too small"):
            _lib.check(_lib.lib.q3_session_decode(s._h, 0, f0, f1, out.ctypes.data_as(ctypes.c_void_p), (f1 - f0) * SPF - 1, ctypes.byref(got)))
        assert got.value == (f1 - f0) * SPF and np.isnan(out).all()
    s.close()
