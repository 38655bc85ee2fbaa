"""Which rows of a ragged first batch share a packed prefill pass: q3_prefill_pack_plan, host arithmetic (no GPU),
plus the ABI of everything the packed pass adds."""
import ctypes
import os
import re

import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L = _lib.lib
INVALID = 1      # Q3_INVALID_ARG
LENS = [10, 16, 609, 47, 48, 1023, 1024, 300, 300]
NEW = ["q3_prefill_pack_plan", "q3_session_prefill_info", "q3_attn_prefill_packed_ex"]


def test_one_pass_in_row_order():
    ps, r0, n = q.prefill_pack_plan(LENS)
    assert n == 1
    # below 48 positions: the decode-step schedule; 1024 and more: the chip alone — both stay in the equal-length groups
    assert [ps[i] for i in (0, 1, 3, 6)] == [-1] * 4 and [r0[i] for i in (0, 1, 3, 6)] == [0] * 4
    packed = [2, 4, 5, 7, 8]
    assert [ps[i] for i in packed] == [0] * 5
    run = 0
    for i in packed:                     # the running sum of the packed lengths, in row order
        assert r0[i] == run
        run += LENS[i]
    assert run == 609 + 48 + 1023 + 300 + 300 <= q.api.PREFILL_PACK_ROWS
    assert q.prefill_pack_plan(LENS, [0] * len(LENS)) == (ps, r0, n)      # no hits = NULL


def test_budget_splits_the_passes():
    ps, r0, n = q.prefill_pack_plan(LENS, row_budget=1000)
    # 609 + 48 = 657; 1023 would pass 1000: the pass closes. 1023 alone; 300 would pass it: closed, alone = no pack. 300 + 300.
    assert n == 2
    assert ps == [-1, -1, 0, -1, 0, -1, -1, 1, 1]
    assert r0 == [0, 0, 0, 0, 609, 0, 0, 0, 300]
    # every pass within the budget, no pass of one row
    for k in range(n):
        rows = [i for i in range(len(LENS)) if ps[i] == k]
        assert len(rows) >= 2 and sum(LENS[i] for i in rows) <= 1000
    # a budget that fits no two rows: nothing packs
    ps, r0, n = q.prefill_pack_plan([300, 300, 300], row_budget=512)
    assert (ps, r0, n) == ([-1] * 3, [0] * 3, 0)
    ps, r0, n = q.prefill_pack_plan([300, 200, 300, 100], row_budget=512)
    assert (ps, r0, n) == ([0, 0, 1, 1], [0, 300, 0, 300], 2)


def test_a_prefix_hit_keeps_the_row_out():
    hits = [0] * len(LENS); hits[4] = 1
    ps, r0, n = q.prefill_pack_plan(LENS, hits)
    assert n == 1 and ps[4] == -1 and r0[4] == 0
    assert [ps[i] for i in (2, 5, 7, 8)] == [0] * 4
    assert [r0[i] for i in (2, 5, 7, 8)] == [0, 609, 609 + 1023, 609 + 1023 + 300]      # the others close up
    # a hit that leaves one row: no pack
    assert q.prefill_pack_plan([300, 200], [2, 0]) == ([-1, -1], [0, 0], 0)


def test_without_the_gemm_path_nothing_packs():
    ps, r0, n = q.prefill_pack_plan(LENS, gemm_ok=False)
    assert (ps, r0, n) == ([-1] * len(LENS), [0] * len(LENS), 0)


def test_refusals():
    i32 = ctypes.c_int32
    ok = (i32 * 3)(100, 200, 300); ps = (i32 * 3)(); r0 = (i32 * 3)(); n = i32(0)
    assert L.q3_prefill_pack_plan(ok, None, 3, 4224, 1, ps, r0, ctypes.byref(n)) == 0 and n.value == 1
    assert L.q3_prefill_pack_plan(ok, None, 3, 4224, 1, ps, r0, None) == 0      # the count is optional
    assert L.q3_prefill_pack_plan(ok, None, 0, 4224, 1, ps, r0, None) == INVALID
    assert L.q3_prefill_pack_plan(ok, None, -1, 4224, 1, ps, r0, None) == INVALID
    assert L.q3_prefill_pack_plan(None, None, 3, 4224, 1, ps, r0, None) == INVALID
    assert L.q3_prefill_pack_plan(ok, None, 3, 4224, 1, None, r0, None) == INVALID
    assert L.q3_prefill_pack_plan(ok, None, 3, 4224, 1, ps, None, None) == INVALID
    assert L.q3_prefill_pack_plan(ok, None, 3, 127, 1, ps, r0, None) == INVALID and b"budget" in L.q3_last_error()
    assert L.q3_prefill_pack_plan(ok, None, 3, 128, 1, ps, r0, None) == 0
    bad = (i32 * 3)(100, 0, 300)
    assert L.q3_prefill_pack_plan(bad, None, 3, 4224, 1, ps, r0, None) == INVALID and b"row 1" in L.q3_last_error()
    hit = (i32 * 3)(0, 0, -1)
    assert L.q3_prefill_pack_plan(ok, hit, 3, 4224, 1, ps, r0, None) == INVALID and b"row 2" in L.q3_last_error()
    with pytest.raises(Exception):
        q.prefill_pack_plan([100, 200], row_budget=64)


def test_new_symbols_are_declared_exported_and_bound():
    hdr = open(os.path.join(ROOT, "include", "q3tts.h")).read()
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", code), f"{name} is not declared in include/q3tts.h"
        assert hasattr(L, name), f"libq3tts.so does not export {name}"
        assert name in _lib.SYMBOLS, f"python binding missing for {name}"
        assert name in doc, f"INTEGRATION.md has no row for {name}"
    assert L.q3_abi_version() == 1                                        # additions only
    # the test entry and the info call refuse null arguments before any device is touched
    assert L.q3_attn_prefill_packed_ex(0, None) == INVALID
    assert L.q3_attn_prefill_packed_ex(0, ctypes.byref(_lib.CAttnPrefillPackedEx())) == INVALID
    assert L.q3_session_prefill_info(None, (ctypes.c_int32 * 8)()) == INVALID
    assert hasattr(q.Session, "prefill_info") and callable(q.prefill_pack_plan) and callable(q.attn_prefill_packed_ex)
