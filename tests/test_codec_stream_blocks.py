"""The block-allocated codec stream (DESIGN 4.3a, q3_codec_stream_create_blocked / _info / _prime): a row's vocoder state lives in
blocks of block_frames frames taken from a free list as the row grows, and reference frames can be given for state only. The
samples stay those of decode_codes over everything the row was given — the same BITS (np.array_equal on float32 PCM; no
tolerance anywhere in this file). Random codes, no talker."""
import ctypes

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib, api
from common import manifest_handle

NEW = ["q3_codec_stream_create_blocked", "q3_codec_stream_info", "q3_codec_stream_prime"]
SPF = 1920
Q3_INVALID_ARG, Q3_OOM = 1, 8


# ---------------------------------------------------------------- no device needed
def test_new_symbols_exported_and_bound():
    for n in NEW:
        assert hasattr(_lib.lib, n), n
        assert n in _lib.SYMBOLS, n
    for n in ("prime", "info"):
        assert callable(getattr(api.CodecStream, n)), n


def test_no_device_no_fallback():
    """Null handles and a manifest-only model (device -1) get a status and a message from every new entry point."""
    L = _lib.lib
    cs = ctypes.c_void_p()
    i = ctypes.c_int(); sz = ctypes.c_size_t()
    frames = (ctypes.c_uint32 * 16)()
    h = manifest_handle(q.tiny())
    assert L.q3_codec_stream_create_blocked(h, 2, 64, 32, 0, ctypes.byref(cs)) != 0
    assert L.q3_last_error() and not cs.value
    L.q3_model_free(h)
    calls = [
        lambda: L.q3_codec_stream_create_blocked(None, 2, 64, 32, 0, ctypes.byref(cs)),
        lambda: L.q3_codec_stream_info(None, ctypes.byref(i), ctypes.byref(sz), ctypes.byref(i), ctypes.byref(i), ctypes.byref(i)),
        lambda: L.q3_codec_stream_prime(None, 0, frames, 1),
    ]
    for k, f in enumerate(calls):
        assert f() != 0, k
        assert L.q3_last_error(), k
    assert not cs.value


@pytest.mark.parametrize("bf", [0, 16, 48, -32])
def test_block_frames_must_be_a_multiple_of_32(bf):
    """Refused before the model is looked at for a device: a manifest-only handle is enough."""
    L = _lib.lib
    h = manifest_handle(q.tiny())
    cs = ctypes.c_void_p()
    assert L.q3_codec_stream_create_blocked(h, 2, 64, bf, 0, ctypes.byref(cs)) == Q3_INVALID_ARG
    assert b"multiple of 32" in L.q3_last_error() and not cs.value
    L.q3_model_free(h)


# ---------------------------------------------------------------- GPU
def _full_decoder_cfg():
    t = q.tiny()
    return q.Q3Config(text_dim=t.text_dim, hidden=t.hidden, inter=t.inter, n_layers=t.n_layers, n_heads=t.n_heads,
                      n_kv_heads=t.n_kv_heads, cp_hidden=t.cp_hidden, cp_inter=t.cp_inter, cp_layers=t.cp_layers,
                      cp_heads=t.cp_heads, cp_kv_heads=t.cp_kv_heads, name="tiny-lm-full-decoder")


@pytest.fixture(scope="module", params=["production", "tiny"])
def dec(request):
    """(model, decode cache): the production decoder shape on the tiny LM and q.tiny()'s. Whole-utterance references are
    computed once per key and shared."""
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


def _ceil(a, b):
    return -(-a // b)


ONE_ROW = [1, 1, 2, 9, 13, 7, 40, 1, 60, 6]


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [32, 64])
def test_one_row_in_pieces(dec, bf):
    """140 frames as 1, 1, 2, 9, 13, 7, 40, 1, 60, 6: crosses frame 12 (stack alone / concatenated); block edges on the 32-query
    tile edges (32) and between them (64); key 128 is wave 0's second key tile, in another block than its first; the first push
    is a single column into a fresh block, and the 60 (frames 74 .. 133) spans three blocks of 32."""
    gm, whole = dec
    assert sum(ONE_ROW) == 140
    codes = _codes(1, 140)
    cs = gm.codec_stream(1, 140, block_frames=bf)
    got, at = [], 0
    for n in ONE_ROW:
        out = cs.push({0: codes[at:at + n]})[0]
        assert out.shape == (n * SPF,)
        got.append(out); at += n
        assert cs.pos(0) == at
        assert cs.info()["blocks_in_use"] == _ceil(at, bf)
    cs.close()
    np.testing.assert_array_equal(np.concatenate(got), whole("one", codes))


@pytest.mark.gpu
def test_single_column_into_a_fresh_block(dec):
    """64 frames, then ONE frame: the only new column is the first of block 2 (block_frames 32), then the rest."""
    gm, whole = dec
    codes = _codes(1, 140)[:80]
    cs = gm.codec_stream(1, 80, block_frames=32)
    got = [cs.push({0: codes[:64]})[0], cs.push({0: codes[64:65]})[0], cs.push({0: codes[65:80]})[0]]
    assert cs.info()["blocks_in_use"] == 3
    cs.close()
    np.testing.assert_array_equal(np.concatenate(got), whole("one80", codes))


@pytest.mark.gpu
def test_first_push_across_a_block_edge(dec):
    """40 frames to a row at frame 0, block_frames 32: the row's stack runs alone on [0, 40), gathered from two blocks."""
    gm, whole = dec
    codes = _codes(1, 140)[:40]
    cs = gm.codec_stream(1, 40, block_frames=32)
    out = cs.push({0: codes})[0]
    assert cs.info()["blocks_in_use"] == 2
    cs.close()
    np.testing.assert_array_equal(out, whole("one40", codes))


def _run(cs, sched, codes, at, got):
    for call in sched:
        out = cs.push({r: codes[r][at[r]:at[r] + n] for r, n in call.items()})
        for r, n in call.items():
            got[r].append(out[r]); at[r] += n


@pytest.mark.gpu
def test_three_rows_reset_and_block_reuse(dec):
    """Three rows at different positions per push (block_frames 32). Row 2 crosses a block edge inside a push (25 -> 45). Row 1 is
    reset at frame 50 and restarted: its two blocks, full of the old sequence, go to the free list and are the next ones taken —
    by row 0 (reaching frame 65) and by row 1's new sequence. Each row equals its own decode_codes: no stale block content shows."""
    gm, whole = dec
    bf = 32
    codes = {0: _codes(20, 75), 1: _codes(21, 50), 2: _codes(22, 85)}
    new1 = _codes(23, 45)
    cs = gm.codec_stream(3, 96, block_frames=bf)
    at = {r: 0 for r in codes}; got = {r: [] for r in codes}
    _run(cs, [{0: 30, 1: 10, 2: 25}, {0: 15, 1: 40, 2: 20}], codes, at, got)
    assert cs.info()["blocks_in_use"] == 2 + 2 + 2
    total = cs.info()["blocks_total"]
    first1 = np.concatenate(got[1])
    cs.reset(1)
    assert cs.pos(1) == 0 and cs.info()["blocks_in_use"] == 4
    codes[1] = new1; at[1] = 0; got[1] = []
    _run(cs, [{0: 20, 1: 5, 2: 7}, {0: 10, 1: 40, 2: 33}], codes, at, got)
    info = cs.info()
    assert info["blocks_in_use"] == sum(_ceil(at[r], bf) for r in at) == 3 + 2 + 3
    assert total == 6 and info["blocks_total"] == 8 and info["blocks_peak"] == 8
    cs.close()
    np.testing.assert_array_equal(first1, whole(("three", "1-old"), _codes(21, 50)))
    np.testing.assert_array_equal(np.concatenate(got[0]), whole(("three", 0), codes[0]))
    np.testing.assert_array_equal(np.concatenate(got[1]), whole(("three", "1-new"), new1))
    np.testing.assert_array_equal(np.concatenate(got[2]), whole(("three", 2), codes[2]))


@pytest.mark.gpu
@pytest.mark.parametrize("bf", [32, 0])
@pytest.mark.parametrize("n_ref", [20, 5])
def test_prime_then_push(dec, bf, n_ref):
    """Reference frames for state only, then 3 + 10 + 25 frames: decode_codes(ref | gen) with the reference's samples cut. With 5
    reference frames the row is still inside its first 12 frames at its first sample (its stack runs alone on [0, e))."""
    gm, whole = dec
    allc = _codes(30 + n_ref, n_ref + 38)
    cs = gm.codec_stream(2, 64, block_frames=bf)
    cs.push({1: allc[:7]})                                   # another row is busy beside it
    cs.prime(0, allc[:n_ref])
    assert cs.pos(0) == n_ref
    with pytest.raises(_lib.Q3Error) as e:                   # state-only frames come first
        cs.prime(0, allc[:3])
    assert e.value.status == Q3_INVALID_ARG and cs.pos(0) == n_ref
    got, at = [], n_ref
    for n in (3, 10, 25):
        got.append(cs.push({0: allc[at:at + n]})[0]); at += n
    if bf:
        assert cs.info()["blocks_in_use"] == _ceil(at, bf) + 1
    else:
        assert cs.info()["block_frames"] == 0
    cs.close()
    np.testing.assert_array_equal(np.concatenate(got), whole(("prime", n_ref), allc)[n_ref * SPF:])


@pytest.mark.gpu
def test_block_figures(dec):
    gm, _ = dec
    bf = 32
    codes = _codes(40, 70)
    cs = gm.codec_stream(3, 96, block_frames=bf)
    info = cs.info()
    assert info["block_frames"] == bf and info["blocks_in_use"] == 0 and info["blocks_total"] == 0
    c = gm.config
    assert info["block_bytes"] == (c.dec_layers * 2 * c.dec_heads * c.dec_head_dim + c.dec_latent) * bf * 4
    pos = {0: 0, 1: 0, 2: 0}
    for call in [{0: 31}, {0: 1, 1: 33}, {0: 1, 2: 70}, {1: 31}, {1: 1}]:
        cs.push({r: codes[pos[r]:pos[r] + n] for r, n in call.items()})
        for r, n in call.items():
            pos[r] += n
        assert cs.info()["blocks_in_use"] == sum(_ceil(p, bf) for p in pos.values())
    assert cs.info()["blocks_in_use"] == 2 + 3 + 3
    cs.reset(2)
    info = cs.info()
    assert info["blocks_in_use"] == 5 and info["blocks_peak"] == 8 and info["blocks_total"] == 8
    cs.push({2: codes[:64]})                                 # two of the three returned blocks are taken again
    info = cs.info()
    assert info["blocks_in_use"] == 7 and info["blocks_peak"] == 8 and info["blocks_total"] == 8
    cs.close()


@pytest.mark.gpu
def test_max_blocks_refusal_changes_nothing(dec):
    """Three blocks of 32. Row 0 holds two (40 frames), row 1 one (20). A push that takes row 1 to 40 frames needs a fourth: Q3_OOM,
    every position as before — also row 0's, which the same push carried. After row 0 is reset the same push goes through."""
    gm, whole = dec
    codes = _codes(1, 140)[:40]
    cs = gm.codec_stream(2, 64, block_frames=32, max_blocks=3)
    a = cs.push({0: codes[:40], 1: codes[:20]})
    assert cs.info()["blocks_in_use"] == 3
    with pytest.raises(_lib.Q3Error) as e:
        cs.push({1: codes[20:40]})
    assert e.value.status == Q3_OOM and "block" in str(e.value)
    assert cs.pos(0) == 40 and cs.pos(1) == 20 and cs.info()["blocks_in_use"] == 3
    cs.reset(0)
    b = cs.push({1: codes[20:40]})
    assert cs.pos(1) == 40 and cs.info()["blocks_in_use"] == 2 and cs.info()["blocks_total"] == 3
    cs.close()
    full = whole("one40", codes)
    np.testing.assert_array_equal(a[0], full)
    np.testing.assert_array_equal(np.concatenate([a[1], b[1]]), full)
