"""What tests/test_gpu_prompt_rows.py rests on and a CPU can check: the references do what they claim, the chosen inputs make the
order of the ICL chain visible in the bits, the tables reach every branch, and q3_prompt_rows_ex refuses — before a device is
touched (status 1, not 5) — everything a kernel could not address."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd import _lib
from qwen3_tts_rs_amd.api import ROWS_GATHER, ROWS_ASSEMBLE, ROWS_COPY, ROWS_SCATTER, ROWS_PUBLISH
import prompt_rows_cases as P

INVALID, NO_DEVICE = 1, 5


def test_tables_reach_every_branch():
    assert P.WIDTHS == (8, 255, 256, 257, 1024) and P.GUARD == q.api.ROWS_GUARD == 64
    combos = {(tr >= 0, "id" if cid >= 0 else cid) for (tr, cid) in P.ASSEMBLE_ROWS if cid >= -3 or cid == -3 - (P.N_REF - 1)}
    assert combos == {(t, c) for t in (True, False) for c in ("id", -1, -2, -3, -3 - (P.N_REF - 1))}
    for n in (1, 5):
        table, ids = P.gather_case(n, 8)
        assert ids.size == n and ids.max() == P.VOCAB - 1 and (n == 1 or (ids.min() == 0 and len(set(ids.tolist())) < n))
    d = P.SCATTER_DST
    assert d.size == 8 and (d == -1).sum() == 3 and {0, P.SCATTER_ROWS - 1} <= set(d.tolist()) and not (np.diff(d[d >= 0]) > 0).all()
    for n in P.PUBLISH_N:
        ent = P.publish_case(n)
        assert ent.shape == (n, 4) and len(set(ent[:, 0].tolist())) == n and ent[:, 0].max() == P.PUBLISH_ROWS - 1
    c = P.assemble_case(8)
    assert c["ref_codes"][:, 0].max() == P.VOCAB - 1 and c["ref_codes"][:, 1:].max() == P.CP_VOCAB - 1


def test_bf16_widening_is_a_shift():
    bits = np.array([0x0000, 0x8000, 0x3f80, 0xbf80, 0x0001, 0x7f7f, 0x4049], dtype=np.uint16)
    assert (P.bf16_to_f32(bits).view(np.uint32) == bits.astype(np.uint32) << 16).all()
    assert P.bf16_to_f32(np.uint16(0x3f80)) == 1.0 and P.bf16_to_f32(np.uint16(0x4049)) == np.float32(3.140625)


@pytest.mark.parametrize("H", P.WIDTHS)
def test_assemble_reference_and_the_power_of_its_bits(H):
    """the reference against plain Python floats (float64 adds of float32 values rounded back are the float32 adds), and: a
    right-to-left chain and a pairwise chain each change at least one output bit, so a reordered or contracted sum cannot pass"""
    c = P.assemble_case(H)
    want = P.assemble_reference(c)
    for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS):
        for col in (0, H - 1):
            if cid >= 0:
                cv = float(P.bf16_to_f32(c["codec_emb"][cid, col]))
            elif cid == -2:
                cv = float(c["xvec"][col])
            elif cid <= -3:
                terms = [float(t[col]) for t in P.icl_terms(c, -3 - cid)]
                cv = terms[0]
                for t in terms[1:]:
                    cv = float(np.float32(cv + t))          # two float32 values add exactly in float64; the rounding back is the float32 add
            else:
                cv = 0.0
            v = float(np.float32(float(c["rows"][tr, col]) + cv)) if tr >= 0 and cid != -1 else (float(c["rows"][tr, col]) if tr >= 0 else cv)
            assert np.float32(v).view(np.uint32) == want[i, col].view(np.uint32), (i, tr, cid, col)
    none = [i for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS) if tr < 0 and cid == -1]
    assert none and all((want[i].view(np.uint32) == 0).all() for i in none), "no text row and no codec part must give +0.0"
    icl = [i for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS) if cid <= -3]
    for name, chain in (("right to left", P.chain_right), ("pairwise", P.chain_pairwise)):
        other = P.assemble_reference(c, chain)
        assert not P.same_bits(other[icl], want[icl]), f"H={H}: a {name} chain gives the same bits on these inputs"
        rest = [i for i in range(len(P.ASSEMBLE_ROWS)) if i not in icl]
        assert P.same_bits(other[rest], want[rest])
    # the two-term adds are where a value is rounded at all: text + codec differs from either part
    both = [i for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS) if tr >= 0 and cid != -1]
    assert all(not P.same_bits(want[i], c["rows"][P.ASSEMBLE_ROWS[i][0]]) for i in both)


def test_copy_scatter_publish_references():
    src, ldd = P.copy_case(3, 255)
    want = P.copy_reference(src, 255, ldd)
    assert src.shape[1] != ldd and P.same_bits(want[:, :255], src[:, :255]) and (want[:, 255:] == P.SENT).all()
    s = P.scatter_case(8)
    w = P.scatter_reference(s, 8)
    assert P.same_bits(w[10], s[0]) and P.same_bits(w[0], s[3]) and (w[[1, 2, 4, 6, 8, 9]] == P.SENT).all()
    ent = P.publish_case(65)
    tl, tr, lim = P.publish_reference(ent)
    assert (tl != P.SENT_I).sum() == 65 and tl[ent[64, 0]] == ent[64, 1] and tr[ent[0, 0]] == ent[0, 2] and lim[ent[7, 0]] == ent[7, 3]


def _status(fn):
    try:
        fn()
    except _lib.Q3Error as e:
        return e.status
    raise AssertionError("the entry returned success without a GPU")


def _gather(**kw):
    table, ids = P.gather_case(5, 8)
    a = dict(table=table, ids=ids, cols=8, out=P.guarded(5 * 8)); a.update(kw)
    return _status(lambda: q.prompt_rows_ex(ROWS_GATHER, **a))


def _assemble(text_row=None, codec_id=None, **kw):
    c = P.assemble_case(8)
    tr = np.array(c["text_row"] if text_row is None else text_row, dtype=np.int32)
    ci = np.array(c["codec_id"] if codec_id is None else codec_id, dtype=np.int32)
    a = dict(src=c["rows"], table=c["codec_emb"], text_row=tr, codec_id=ci, xvec=c["xvec"], ref_codes=c["ref_codes"], cp_embs=c["cp_embs"], cols=8,
             out=P.guarded(tr.size * 8))
    a.update(kw)
    return _status(lambda: q.prompt_rows_ex(ROWS_ASSEMBLE, **a))


def test_entry_refuses_what_a_kernel_could_not_address():
    """every refusal is Q3_INVALID_ARG (1), decided before the device is asked for; the same calls with good arguments get as far
    as the device (5 on a machine without one; with a GPU the good calls are test_gpu_prompt_rows.py's)."""
    have_gpu = _lib.lib.q3_device_count() > 0
    ok = lambda st: st == NO_DEVICE
    # gather: an id outside the table
    assert _gather(ids=np.array([0, 1, P.VOCAB, 2, 3], dtype=np.uint32)) == INVALID
    assert _gather(ids=np.array([0, 1, 0xffffffff, 2, 3], dtype=np.uint32)) == INVALID
    # assemble: rows / ids outside their table, an ICL frame beyond ref_codes, codes outside their tables, -2 without xvec
    assert _assemble(text_row=[P.N_TEXT], codec_id=[0]) == INVALID
    assert _assemble(text_row=[0], codec_id=[P.VOCAB]) == INVALID
    assert _assemble(text_row=[0], codec_id=[-3 - P.N_REF]) == INVALID
    assert _assemble(text_row=[0], codec_id=[-(1 << 31)]) == INVALID
    assert _assemble(text_row=[0], codec_id=[-3], ref_codes=None) == INVALID
    assert _assemble(text_row=[0], codec_id=[-3], cp_embs=None) == INVALID
    assert _assemble(text_row=[0], codec_id=[-2], xvec=None) == INVALID
    bad = P.assemble_case(8)["ref_codes"].copy(); bad[1, 0] = P.VOCAB
    assert _assemble(text_row=[0], codec_id=[-4], ref_codes=bad) == INVALID
    bad = P.assemble_case(8)["ref_codes"].copy(); bad[1, 15] = P.CP_VOCAB
    assert _assemble(text_row=[0], codec_id=[-4], ref_codes=bad) == INVALID
    # copy: a pitch below cols
    src, ldd = P.copy_case(3, 8)
    assert _status(lambda: q.prompt_rows_ex(ROWS_COPY, src=src, cols=12, ldd=16, out=P.guarded(3 * 16))) == INVALID
    assert _status(lambda: q.prompt_rows_ex(ROWS_COPY, src=src, cols=8, ldd=7, out=P.guarded(3 * 7))) == INVALID
    # scatter: a row outside `rows`, a destination named twice
    s = P.scatter_case(8)
    sc = lambda dst: _status(lambda: q.prompt_rows_ex(ROWS_SCATTER, src=s, dst_row=np.array(dst, dtype=np.int32), cols=8, n_rows=P.SCATTER_ROWS,
                                                      out=P.guarded(P.SCATTER_ROWS * 8)))
    assert sc([10, -1, 3, 0, -1, 7, -1, P.SCATTER_ROWS]) == INVALID
    assert sc([10, -1, 3, 0, -1, 7, -1, 3]) == INVALID
    # publish: a row outside the arrays (negative too), a row named twice
    def pub(ent):
        arrs = [P.guarded(P.PUBLISH_ROWS, np.int32) for _ in range(3)]
        return _status(lambda: q.prompt_rows_ex(ROWS_PUBLISH, ent=np.array(ent, dtype=np.int32), n_rows=P.PUBLISH_ROWS, trail_len=arrs[0], text_ready=arrs[1],
                                                limit=arrs[2]))
    assert pub([[P.PUBLISH_ROWS, 1, 2, 3]]) == INVALID and pub([[-1, 1, 2, 3]]) == INVALID
    assert pub([[4, 1, 2, 3], [5, 1, 2, 3], [4, 7, 8, 9]]) == INVALID
    # shapes
    assert _gather(cols=0, table=np.zeros((P.VOCAB, 0), np.uint16), out=P.guarded(0)) == INVALID
    a = _lib.CPromptRowsEx(); a.mode = 5
    assert _lib.lib.q3_prompt_rows_ex(0, a) == INVALID
    if not have_gpu:
        assert ok(_gather()) and ok(_assemble()) and ok(sc(P.SCATTER_DST)) and ok(pub(P.publish_case(65)))
        assert ok(_status(lambda: q.prompt_rows_ex(ROWS_COPY, src=src, cols=8, ldd=ldd, out=P.guarded(3 * ldd))))
