"""The codec stream (DESIGN 4.3a, q3_codec_stream_*): the vocoder with per-row state. Frames appended to a row in pieces, beside
other rows at other positions in the same decode pass, must give the samples of decode_codes over everything the row was
given — the same BITS (np.array_equal on float32 PCM; no tolerance anywhere in this file). Random codes, no talker."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import manifest_handle

NEW = ["q3_codec_stream_create", "q3_codec_stream_free", "q3_codec_stream_reset", "q3_codec_stream_pos", "q3_codec_stream_push",
       "q3_session_next_chunks"]
SPF = 1920


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    assert _lib.lib.q3_abi_version() == 1
    assert callable(api.Qwen3TTS.codec_stream) and callable(api.Session.next_chunks)
    for n in ("push", "reset", "pos", "close"):
        assert callable(getattr(api.CodecStream, n)), n


def test_no_device_no_fallback():
    """A manifest-only model (device -1) has no vocoder: the new entry points refuse it with a status and a message, they do
    not route anywhere else (the pattern of test_abi.py::test_no_cpu_fallback)."""
    L = _lib.lib
    h = manifest_handle(q.tiny())
    cs = ctypes.c_void_p()
    assert L.q3_codec_stream_create(h, 2, 16, ctypes.byref(cs)) != 0
    assert L.q3_last_error() and not cs.value
    L.q3_model_free(h)
    i = ctypes.c_int(); sz = ctypes.c_size_t()
    calls = [
        lambda: L.q3_codec_stream_create(None, 2, 16, ctypes.byref(cs)),
        lambda: L.q3_codec_stream_reset(None, 0),
        lambda: L.q3_codec_stream_pos(None, 0, ctypes.byref(i)),
        lambda: L.q3_codec_stream_push(None, 0, None, None, None, None, None),
        lambda: L.q3_session_next_chunks(None, None, None, ctypes.byref(sz), ctypes.byref(i)),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error(), k
    L.q3_codec_stream_free(None)      # free(NULL) is a no-op


# ---------------------------------------------------------------- GPU
def _full_decoder_cfg():
    t = q.tiny()
    return q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads,
                      n_kv_heads=t.n_kv_heads, cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers,
                      cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads, name="tiny-lm-full-decoder")


@pytest.fixture(scope="module", params=["production", "tiny"])
def dec(request):
    """(model, decode cache): the production decoder (bf16x3 kernels) and q.tiny()'s (the fallback kernels). Whole-utterance
    references are computed once per (codes, planes) and shared."""
    gm = q.Qwen3TTS.from_synthetic(_full_decoder_cfg() if request.param == "production" else q.tiny())
    cache = {}

    def whole(key, codes):
        if key not in cache:
            cache[key] = gm.decode_codes(codes).samples.copy()
        return cache[key]
    yield gm, whole
    gm.close()


def _codes(seed, n):
    return np.random.default_rng(seed).integers(0, 2048, size=(n, 16)).astype(np.uint32)


ONE_ROW = [1, 1, 2, 9, 13, 7, 40, 1, 60, 6]


@pytest.mark.gpu
def test_one_row_in_pieces(dec):
    """140 frames as 1, 1, 2, 9, 13, 7, 40, 1, 60, 6: crosses frame 12 (stack alone / concatenated), single-column pushes, the
    32-query tile edges at 32 / 64 / 96 / 128, key 128 (wave 0's second key tile), a push longer than the context and than
    32 columns."""
    gm, whole = dec
    assert sum(ONE_ROW) == 140
    codes = _codes(1, 140)
    cs = gm.codec_stream(1, 140)
    got, at = [], 0
    for n in ONE_ROW:
        out = cs.push({0: codes[at:at + n]})[0]
        assert out.shape == (n * SPF,)
        got.append(out); at += n
        assert cs.pos(0) == at
    cs.close()
    np.testing.assert_array_equal(np.concatenate(got), whole("one", codes))


# calls of the three-row schedule: {row: frames in this call}. Row 0 pushes 10 per call; row 1 joins when row 0 is at 30 (a row
# start beside running rows); row 2 pushes 33 per call; some calls lack a row and call 5 carries a single row of 10 columns,
# so the columns per call fall on both sides of 32 (10 ... 53).
THREE_ROWS = [{0: 10, 2: 33}, {0: 10}, {0: 10, 2: 33}, {0: 10, 1: 7, 2: 33}, {1: 10, 2: 33}, {0: 10}, {0: 10, 1: 10}, {1: 20, 2: 8}]


def _run_schedule(cs, sched, codes, at=None, got=None):
    at = at if at is not None else {r: 0 for r in codes}
    got = got if got is not None else {r: [] for r in codes}
    for call in sched:
        out = cs.push({r: codes[r][at[r]:at[r] + n] for r, n in call.items()})
        for r, n in call.items():
            assert out[r].shape == (n * SPF,)
            got[r].append(out[r]); at[r] += n
    return at, got


def _three_row_codes():
    tot = {r: sum(c.get(r, 0) for c in THREE_ROWS) for r in range(3)}
    return {r: _codes(10 + r, tot[r]) for r in range(3)}


@pytest.mark.gpu
def test_three_rows_out_of_phase(dec):
    gm, whole = dec
    codes = _three_row_codes()
    cs = gm.codec_stream(3, 160)
    at, got = _run_schedule(cs, THREE_ROWS, codes)
    cs.close()
    for r in range(3):
        assert at[r] == len(codes[r])
        np.testing.assert_array_equal(np.concatenate(got[r]), whole(("three", r), codes[r]))


@pytest.mark.gpu
def test_reset_one_row_in_mid_sequence(dec):
    """Row 2 is reset after three calls and starts another sequence at frame 0 beside rows 0 and 1, which go on undisturbed."""
    gm, whole = dec
    codes = _three_row_codes()
    cs = gm.codec_stream(3, 160)
    at, got = _run_schedule(cs, THREE_ROWS[:3], codes)
    assert cs.pos(2) == 66
    cs.reset(2)
    assert cs.pos(2) == 0 and cs.pos(0) == 30
    new2 = _codes(99, 33 + 33 + 8)
    codes2 = {0: codes[0], 1: codes[1], 2: new2}
    at[2] = 0; got[2] = []
    at, got = _run_schedule(cs, THREE_ROWS[3:], codes2, at, got)
    cs.close()
    for r in (0, 1):
        np.testing.assert_array_equal(np.concatenate(got[r]), whole(("three", r), codes[r]))
    np.testing.assert_array_equal(np.concatenate(got[2]), whole("reset2", new2))


@pytest.mark.gpu
def test_three_rows_two_planes(dec):
    """set_codec_planes(2) applies to the stream as it does to decode_codes."""
    gm, whole = dec
    codes = _three_row_codes()
    gm.set_codec_planes(2)
    try:
        cs = gm.codec_stream(3, 160)
        at, got = _run_schedule(cs, THREE_ROWS, codes)
        cs.close()
        for r in range(3):
            np.testing.assert_array_equal(np.concatenate(got[r]), whole(("three-2planes", r), codes[r]))
    finally:
        gm.set_codec_planes(3)


@pytest.mark.gpu
def test_refusals_change_nothing(dec):
    gm, whole = dec
    codes = _codes(1, 140)
    cs = gm.codec_stream(2, 40)
    a = cs.push({0: codes[:9], 1: codes[:5]})
    bad = [
        lambda: cs._push_lists([0, 2], [codes[9:12], codes[:3]]),                      # row out of range
        lambda: cs._push_lists([-1], [codes[:3]]),
        lambda: cs._push_lists([0, 0], [codes[9:12], codes[12:15]]),                  # duplicate row
        lambda: cs._push_lists([1, 0], [codes[5:8], codes[9:41]]),                    # past max_frames (row 0: 9 + 32 > 40)
        lambda: cs._push_lists([1, 0], [codes[5:8], codes[9:12]], cap=[3 * SPF, 3 * SPF - 1]),      # cap too small
    ]
    for k, f in enumerate(bad):
        with pytest.raises(_lib.Q3Error) as e:
            f()
        assert e.value.status == 1, k
        assert cs.pos(0) == 9 and cs.pos(1) == 5, k
    assert cs._push_lists([1, 0], [codes[5:5], codes[9:9]]) is not None and cs.pos(0) == 9       # n = 0: a no-op
    b = cs.push({0: codes[9:40], 1: codes[5:40]})
    cs.close()
    full = whole("one40", codes[:40])
    np.testing.assert_array_equal(np.concatenate([a[0], b[0]]), full)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), full)


@pytest.mark.gpu
def test_not_vacuous(dec):
    """The context-free decodes of the same pieces, concatenated, differ from the whole decode: equality above is the state's doing."""
    gm, whole = dec
    codes = _codes(1, 140)
    parts, at = [], 0
    for n in ONE_ROW:
        parts.append(gm.decode_codes(codes[at:at + n]).samples); at += n
    free = np.concatenate(parts)
    full = whole("one", codes)
    assert free.shape == full.shape and not np.array_equal(free, full)


@pytest.mark.gpu
def test_sixty_four_rows_chunk_ten(dec):
    """The width the stream is for: 64 rows, 13 frames each (every row's stack alone), then twice 10 each in one push — the
    front over N = 640 new columns, the stack over Lc = 64 * 22 = 1408 concatenated ones, the sizes at which the linears and
    convs pick their wide geometries. Every row against its own whole decode."""
    gm, whole = dec
    R = 64
    codes = {r: _codes(200 + r, 33) for r in range(R)}
    cs = gm.codec_stream(R, 33)
    at, got = _run_schedule(cs, [{r: 13 for r in range(R)}, {r: 10 for r in range(R)}, {r: 10 for r in range(R)}], codes)
    cs.close()
    for r in range(R):
        np.testing.assert_array_equal(np.concatenate(got[r]), whole(("wide", r), codes[r]), err_msg=f"row {r}")
