"""The row-state kernel at op level (k_row_move through q3_row_move): one launch over a list of byte segments, copy
or exchange, any length and alignment. Every result is compared with a numpy restatement over the WHOLE buffers, so the bytes
around every destination (the guards) are checked too — np.array_equal, no tolerance."""
import ctypes
import itertools

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib

Q3_INVALID_ARG = 1
COPY, EXCHANGE = 0, 1
LENGTHS = [0, 1, 3, 15, 16, 17, 4097, 65536 + 5]
OFFSETS = [0, 4, 1]          # bytes past a 16-byte boundary: equal offsets take the vector path, 0/4 the word path, the rest bytes
GUARD = 48


# ---------------------------------------------------------------- no device needed
def test_symbol_exported_and_bound():
    assert hasattr(_lib.lib, "q3_row_move") and "q3_row_move" in _lib.SYMBOLS
    assert callable(q.row_move)


def test_bad_arguments_return_status():
    L = _lib.lib
    buf = (ctypes.c_uint8 * 64)()
    one = (ctypes.c_size_t * 1)(0); n = (ctypes.c_size_t * 1)(16); far = (ctypes.c_size_t * 1)(60); mode = (ctypes.c_int * 1)(0); bad = (ctypes.c_int * 1)(7)
    calls = [
        lambda: L.q3_row_move(0, None, 64, buf, 64, 1, one, one, n, mode),
        lambda: L.q3_row_move(0, buf, 64, buf, 64, 0, one, one, n, mode),
        lambda: L.q3_row_move(0, buf, 64, buf, 64, 1, one, one, n, None),
        lambda: L.q3_row_move(0, buf, 64, buf, 64, 1, far, one, n, mode),          # 16 bytes from offset 60 of 64: leaves the source
        lambda: L.q3_row_move(0, buf, 64, buf, 64, 1, one, far, n, mode),          # ... the destination
        lambda: L.q3_row_move(0, buf, 64, buf, 64, 1, one, one, n, bad),
    ]
    for k, f in enumerate(calls):
        assert f() == Q3_INVALID_ARG, k
        assert _lib.lib.q3_last_error(), k


# ---------------------------------------------------------------- GPU
def _restate(src, dst, segs):
    s, d = src.copy(), dst.copy()
    for so, do, n, mode in segs:
        a, b = s[so:so + n].copy(), d[do:do + n].copy()
        d[do:do + n] = a
        if mode == EXCHANGE:
            s[so:so + n] = b
    return s, d


def _layout(cases, mode):
    """segments laid out one after the other in two buffers: each starts `offset` bytes past a 16-byte boundary, with GUARD
    bytes around it"""
    segs, s_at, d_at = [], GUARD, GUARD
    for n, so, do in cases:
        s_at = (s_at + 15) // 16 * 16; d_at = (d_at + 15) // 16 * 16
        segs.append((s_at + so, d_at + do, n, mode))
        s_at += so + n + GUARD; d_at += do + n + GUARD
    return segs, s_at + GUARD, d_at + GUARD


def _check(cases, mode, seed):
    segs, ns, nd = _layout(cases, mode)
    rng = np.random.default_rng(seed)
    src = rng.integers(0, 256, ns, dtype=np.uint8); dst = rng.integers(0, 256, nd, dtype=np.uint8)
    want_s, want_d = _restate(src, dst, segs)
    got_s, got_d = q.row_move(src, dst, segs)
    assert np.array_equal(got_d, want_d), "destination (guards included)"
    assert np.array_equal(got_s, want_s), "source"
    if mode == EXCHANGE:                             # an exchange applied twice restores both buffers
        back_s, back_d = q.row_move(got_s, got_d, segs)
        assert np.array_equal(back_s, src) and np.array_equal(back_d, dst)


ALL_CASES = list(itertools.product(LENGTHS, OFFSETS, OFFSETS))


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [COPY, EXCHANGE])
def test_one_segment_per_launch(mode):
    """every length x source offset x destination offset, one segment in its launch"""
    for k, case in enumerate(ALL_CASES):
        _check([case], mode, 100 + k)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [COPY, EXCHANGE])
def test_forty_segments_in_one_launch(mode):
    """40 segments of every length and alignment pair in ONE launch (the grid is sized for the longest: the short ones' spare
    blocks must write nothing)"""
    cases = [ALL_CASES[(7 * k) % len(ALL_CASES)] for k in range(40)]
    assert {c[0] for c in cases} == set(LENGTHS)
    _check(cases, mode, 7)


@pytest.mark.gpu
def test_mixed_modes_in_one_launch():
    segs, ns, nd = _layout([(4097, 0, 0), (17, 1, 4), (16, 4, 4), (65541, 4, 0)], COPY)
    segs = [(so, do, n, k % 2) for k, (so, do, n, _m) in enumerate(segs)]
    rng = np.random.default_rng(3)
    src = rng.integers(0, 256, ns, dtype=np.uint8); dst = rng.integers(0, 256, nd, dtype=np.uint8)
    want_s, want_d = _restate(src, dst, segs)
    got_s, got_d = q.row_move(src, dst, segs)
    assert np.array_equal(got_s, want_s) and np.array_equal(got_d, want_d)
