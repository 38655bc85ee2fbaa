"""Park and resume at the session level (DESIGN 4.13, q3_session_park_row / _resume_row / q3_parked_*): a running row's state
leaves the session between two frames and enters a row of it again later. Every comparison is np.array_equal against THE SAME
SESSION RUN WITHOUT PARKS (today's code path), computed once per module — never against another parked run. Tiny LM with the
production decoder shape; rows: CustomVoice greedy, VoiceDesign with a 130-token instruct sampled at T = 0.9 (two prompt pages),
ICL with 5 reference frames."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import synthetic_prompt
from test_batcher_stream import _full_decoder_cfg

NEW = ["q3_session_park_row", "q3_session_resume_row", "q3_parked_free", "q3_parked_info"]
Q3_INVALID_ARG, Q3_UNSUPPORTED = 1, 7
PATHS = ["aql", "hipgraph", "eager"]
LIMITS = [10, 30, 24]
HOST = dict(eos_token_id=None, max_length=32, seed=1)


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_declared_and_bound():
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "q3tts.h")).read()
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
        assert n + "(" in hdr, n
    assert "typedef struct q3_parked q3_parked;" in hdr


def test_null_handles_and_bad_arguments_return_status():
    L = _lib.lib
    h = ctypes.c_void_p(); i = ctypes.c_int()
    calls = [
        lambda: L.q3_session_park_row(None, 0, ctypes.byref(h)),
        lambda: L.q3_session_resume_row(None, 0, None),
        lambda: L.q3_parked_info(None, ctypes.byref(i), None, None, None, None),
    ]
    for k, f in enumerate(calls):
        assert f() == Q3_INVALID_ARG, k
        assert L.q3_last_error(), k
    L.q3_parked_free(None)                            # free(NULL) is a no-op


def test_python_surface():
    for n in ("park_row", "resume_row"):
        assert callable(getattr(api.Session, n)), n
    for n in ("info", "free"):
        assert callable(getattr(api.Parked, n)), n
    assert q.Parked is api.Parked


# ---------------------------------------------------------------- GPU
def _path(monkeypatch, path):
    if path == "hipgraph":
        monkeypatch.setenv("Q3_AQL", "0")
    else:
        monkeypatch.delenv("Q3_AQL", raising=False)
    return path != "eager"


def _utts(cfg, eos1=None, limits=LIMITS, n_instruct=130):
    rng = np.random.default_rng(11)
    xv = rng.standard_normal(cfg.hidden).astype(np.float32)
    ref = rng.integers(0, 2048, size=(5, 16)).astype(np.uint32)
    u0 = q.Utterance(synthetic_prompt(9, 0), q.Speaker.Ryan, q.Language.English, seed=42)
    u0.options = q.SynthesisOptions(temperature=0.0, **HOST)
    u1 = q.Utterance(synthetic_prompt(8, 1), language=q.Language.German, instruct_ids=synthetic_prompt(n_instruct, 51), seed=43)
    u1.options = q.SynthesisOptions(temperature=0.9, **dict(HOST, eos_token_id=eos1))
    u2 = q.Utterance(synthetic_prompt(11, 2), language=q.Language.French, xvector=xv, ref_codes=ref, ref_text_ids=synthetic_prompt(3, 94), seed=44)
    u2.options = q.SynthesisOptions(temperature=0.9, **HOST)
    utts = [u0, u1, u2]
    for u, L in zip(utts, limits):
        u.max_length = L
    return utts


def _session(gm, utts, **kw):
    s = gm.session(utts, q.SynthesisOptions(**HOST), **kw)
    s.prefill()
    return s


def _result(s, rows):
    return [(s.codes(b), s.decode(b)) for b in rows]


@pytest.fixture(scope="module")
def world():
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg(), seed=1234)
    utts = _utts(gm.config)
    pages0 = gm.kv_pool_info()["pages_in_use"]
    s = _session(gm, utts)
    assert s.prefill_len(1)[0] > 128                 # two prompt pages
    s.generate(100)
    want = _result(s, range(3))
    s.close()
    for (codes, _pcm), L in zip(want, LIMITS):
        assert codes.shape == (L, 16)
    assert gm.kv_pool_info()["pages_in_use"] == pages0
    yield gm, utts, want, pages0
    gm.close()


def _same(got, want, what):
    np.testing.assert_array_equal(got[0], want[0], err_msg=f"{what}: codes")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: PCM")


@pytest.mark.gpu
@pytest.mark.parametrize("path", PATHS)
def test_park_and_resume_into_the_same_row(world, monkeypatch, path):
    gm, utts, want, _ = world
    g = _path(monkeypatch, path)
    s = _session(gm, utts)
    s.generate(7, g)
    p = s.park_row(1)
    info = p.info()
    assert info["frames_committed"] == 7 and info["limit"] == 30 and not info["done"] and info["kv_pages"] == 2 and info["state_bytes"] > 0
    s.generate(5, g)
    assert s.frames(0) == (10, True) and s.frames(2) == (12, False)
    s.resume_row(1, p)
    assert p._h is None and s.frames(1) == (7, False)
    s.generate(100, g)
    for b in range(3):
        _same(_result(s, [b])[0], want[b], f"row {b}")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("row", [1, 2])
@pytest.mark.parametrize("path", PATHS)
def test_resume_into_another_row(world, monkeypatch, path, row):
    """row 1 (two prompt pages) or row 2 (ICL: its reference frames travel with it) goes on in row 0, which has ended meanwhile"""
    gm, utts, want, _ = world
    g = _path(monkeypatch, path)
    s = _session(gm, utts)
    s.generate(7, g)
    p = s.park_row(row)
    s.generate(5, g)
    assert s.frames(0) == (10, True)
    s.resume_row(0, p)
    s.generate(100, g)
    other = 3 - row
    _same(_result(s, [0])[0], want[row], f"row {row} resumed into row 0")
    _same(_result(s, [other])[0], want[other], f"row {other}")
    s.close()


@pytest.mark.gpu
def test_park_twice_across_page_boundaries(world):
    """A prompt of 120 positions: position 128 is reached at frame 8, position 256 at frame 136. Parks at frames 5 and 12 (the
    first boundary lies between them, the second page taken while the row sat in row 0), the third page is taken after the
    second resume, back in row 1."""
    gm, _, _, _ = world
    utts = _utts(gm.config, limits=[4, 150, 20], n_instruct=111)
    host = q.SynthesisOptions(**dict(HOST, max_length=150))

    def run(parks):
        s = gm.session(utts, host); s.prefill()
        assert s.prefill_len(1)[0] == 120
        if parks:
            s.generate(5)
            p = s.park_row(1); assert p.info()["kv_pages"] == 1
            s.generate(3)
            s.resume_row(0, p)                       # row 0 ended at frame 4
            s.generate(7)
            p = s.park_row(0); assert p.info()["kv_pages"] == 2 and p.info()["frames_committed"] == 12
            s.generate(2)
            s.resume_row(1, p)
        s.generate(200)
        out = _result(s, [1, 2])
        s.close()
        return out

    want, got = run(False), run(True)
    assert want[0][0].shape == (150, 16)
    _same(got[0], want[0], "the long row")
    _same(got[1], want[1], "its neighbour")


def _eos_world(gm, want):
    """a live EOS id for row 1: the semantic code of its frame 15 in the run without EOS, if no earlier frame has it"""
    sem = want[1][0][:, 0]
    f = next(f for f in range(9, 28) if sem[f] not in sem[:f])
    return int(sem[f]), f


@pytest.mark.gpu
@pytest.mark.parametrize("after_eos", [False, True])
def test_live_eos(world, after_eos):
    """Hazard "EOS": the device freezes a row at its limit, not at EOS. A row that ends on EOS after a resume ends at the same
    frame; a row parked AFTER its EOS frame resumes as ended (the record says done) with the same frames."""
    gm, _, want, _ = world
    eos, f_eos = _eos_world(gm, want)
    utts = _utts(gm.config, eos1=eos)
    s = _session(gm, utts); s.generate(100)
    ref = _result(s, range(3)); s.close()
    assert ref[1][0].shape[0] == f_eos and np.array_equal(ref[1][0], want[1][0][:f_eos])      # the run really ends on EOS
    s = _session(gm, utts)
    if after_eos:
        s.generate(f_eos + 2)
        assert s.frames(1) == (f_eos, True)
        p = s.park_row(1)
        assert p.info()["done"] and p.info()["frames_committed"] >= f_eos
        s.resume_row(0, p)
        assert s.frames(0) == (f_eos, True)
        dst = 0
    else:
        s.generate(7); p = s.park_row(1); s.generate(4); s.resume_row(1, p)
        dst = 1
    s.generate(100)
    assert s.frames(dst) == (f_eos, True)
    _same(_result(s, [dst])[0], ref[1], "the EOS row")
    _same(_result(s, [2])[0], ref[2], "row 2")
    s.close()


@pytest.mark.gpu
@pytest.mark.parametrize("record_outlives_session", [False, True])
def test_page_accounting(world, record_outlives_session):
    gm, utts, _, pages0 = world
    s = _session(gm, utts); s.generate(3)
    base = gm.kv_pool_info()["pages_in_use"]
    assert base == pages0 + 4                        # 1 + 2 + 1 prompt pages
    p = s.park_row(1)
    held = p.info()["kv_pages"]
    assert held == 2
    assert gm.kv_pool_info()["pages_in_use"] == base + 1      # the record's pages were the row's; the vacated row holds one of its own
    if record_outlives_session:
        s.close()
        assert gm.kv_pool_info()["pages_in_use"] == pages0 + held
        assert p.info()["frames_committed"] == 3
        p.free()
    else:
        p.free()
        assert gm.kv_pool_info()["pages_in_use"] == base + 1 - held
        s.generate(100)                              # the session goes on without the row
        s.close()
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_prefix_cache_pages_travel(world):
    """The parked row links pages the prefix cache holds too; the cache is sized down to nothing while it is parked."""
    gm, utts, want, pages0 = world
    gm.prefix_cache(64)
    try:
        s = _session(gm, utts); s.close()            # the donor: its instruct pages stay cached
        s = _session(gm, utts)
        assert s.prefix_info(1) >= 128
        s.generate(7)
        p = s.park_row(1)
        gm.prefix_cache(0)
        s.generate(5)
        s.resume_row(0, p)
        s.generate(100)
        _same(_result(s, [0])[0], want[1], "the cached row")
        _same(_result(s, [2])[0], want[2], "row 2")
        s.close()
    finally:
        gm.prefix_cache(0)
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_bf16_kv(world):
    gm, utts, _, pages0 = world

    def run(parks):
        s = _session(gm, utts, kv_bf16=True)
        if parks:
            s.generate(7); p = s.park_row(1); s.generate(5); s.resume_row(0, p)
        s.generate(100)
        out = [s.codes(1 if not parks else 0), s.codes(2)]
        s.close()
        return out

    want, got = run(False), run(True)
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert gm.kv_pool_info()["pages_in_use"] == pages0


@pytest.mark.gpu
def test_seventeen_rows(world):
    """A wide session (the GEMM path): row 16 is parked at frame 3 and goes on in row 2, which ended at frame 2."""
    gm, _, _, _ = world
    utts = []
    for i in range(17):
        u = q.Utterance(synthetic_prompt(6, i), q.Speaker.Ryan, q.Language.English, seed=100 + i)
        u.options = q.SynthesisOptions(temperature=0.0 if i % 2 else 0.9, **HOST)
        u.max_length = 2 if i == 2 else 9 + i % 4
        utts.append(u)

    def run(parks):
        s = _session(gm, utts)
        if parks:
            s.generate(3); p = s.park_row(16); s.generate(2)
            assert s.frames(2) == (2, True)
            s.resume_row(2, p)
        s.generate(100)
        out = [s.codes(b) for b in range(17)]
        s.close()
        return out

    want, got = run(False), run(True)
    np.testing.assert_array_equal(got[2], want[16])
    assert want[16].shape[0] == 9
    for b in range(16):
        if b != 2:
            np.testing.assert_array_equal(got[b], want[b], err_msg=f"row {b}")


def _status(f):
    try:
        f()
    except _lib.Q3Error as e:
        return e.status
    return 0


@pytest.mark.gpu
def test_refusals_change_nothing(world, monkeypatch):
    gm, utts, want, _ = world
    s = _session(gm, utts); s.generate(7)
    other = _session(gm, utts); other.generate(2)
    p = s.park_row(1)
    assert _status(lambda: s.resume_row(2, p)) == Q3_INVALID_ARG           # a live target row
    assert _status(lambda: other.resume_row(0, p)) == Q3_INVALID_ARG       # another session's record (row 0 there is live too: foreign comes first)
    assert _status(lambda: s.park_row(1)) == Q3_INVALID_ARG                # the vacated row is idle
    assert p._h is not None and p.info()["frames_committed"] == 7
    other.close()
    s.generate(5)
    s.resume_row(1, p)
    s.generate(100)
    for b in range(3):
        _same(_result(s, [b])[0], want[b], f"row {b}")
    s.close()
    # a row that has delivered chunks
    s = _session(gm, utts)
    chunk, _done = s.next_chunk_row(2)
    assert chunk is not None
    assert _status(lambda: s.park_row(2)) == Q3_UNSUPPORTED
    s.close()
    # a debug session
    s = gm.session(utts[:1], q.SynthesisOptions(**HOST), debug=True); s.prefill(); s.generate(2, False)
    assert _status(lambda: s.park_row(0)) == Q3_UNSUPPORTED
    s.close()
    # contiguous K/V (read per session)
    monkeypatch.setenv("Q3_KV_CONTIGUOUS", "1")
    s = _session(gm, utts); s.generate(2)
    assert _status(lambda: s.park_row(1)) == Q3_UNSUPPORTED
    s.generate(100)
    np.testing.assert_array_equal(s.codes(1), want[1][0])
    s.close()
