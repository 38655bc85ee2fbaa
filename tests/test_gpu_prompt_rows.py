"""Op-level tests of the kernels that build the prompt rows (-m gpu): k_gather_rows_bf16, k_assemble_rows, k_copy_rows,
k_scatter_rows and k_publish_text of q3_kernels_lm.hip, exactly one launch each through q3_prompt_rows_ex, BIT FOR BIT — the
kernels move rows and add at most two float32 values per element, so the references of prompt_rows_cases.py are exact. Every
destination goes up whole between 64-element guards filled with a sentinel: what a kernel writes outside its rows shows, and so does
a row it leaves out. Widths are 8, 255, 256, 257 and 1024: the edges of the 256-thread stride loop.

What needs no GPU — the references against plain Python floats, the proof that a reordered ICL chain changes bits on these inputs,
the tables, every refusal of the entry — is in test_prompt_rows_reference.py."""
import numpy as np
import pytest

import qwen3_tts_rs_amd as q
from qwen3_tts_rs_amd.api import ROWS_GATHER, ROWS_ASSEMBLE, ROWS_COPY, ROWS_SCATTER, ROWS_PUBLISH
import prompt_rows_cases as P

pytestmark = pytest.mark.gpu


def _guards_intact(buf, what):
    sent = P.SENT if buf.dtype == np.float32 else P.SENT_I
    g = np.concatenate([buf[:P.GUARD], buf[buf.size - P.GUARD:]])
    bad = np.argwhere(g.view(np.uint32) != np.full_like(g, sent).view(np.uint32))
    assert len(bad) == 0, f"{what}: guard element {int(bad[0][0])} of {2 * P.GUARD} written"


def _equal(got, want, what):
    d = P.first_diff(got, want)
    assert d is None, f"{what}: first differing element {d}: {got[d]!r} != {want[d]!r}"


@pytest.mark.parametrize("dim", P.WIDTHS)
@pytest.mark.parametrize("n", [1, 5])
def test_gather_rows_bf16(n, dim):
    table, ids = P.gather_case(n, dim)
    out = q.prompt_rows_ex(ROWS_GATHER, table=table, ids=ids, cols=dim, out=P.guarded(n * dim))
    what = f"k_gather_rows_bf16 n={n} dim={dim}"
    _guards_intact(out, what)
    got = P.payload(out).reshape(n, dim)
    _equal(got, P.gather_reference(table, ids), what)
    assert (got.view(np.uint32) == table[ids].astype(np.uint32) << 16).all(), f"{what}: not bf16 << 16"


@pytest.mark.parametrize("H", P.WIDTHS)
def test_assemble_rows(H):
    """one launch over every (text_row, codec_id) combination"""
    c = P.assemble_case(H)
    n = len(P.ASSEMBLE_ROWS)
    out = q.prompt_rows_ex(ROWS_ASSEMBLE, src=c["rows"], table=c["codec_emb"], text_row=c["text_row"], codec_id=c["codec_id"], xvec=c["xvec"],
                           ref_codes=c["ref_codes"], cp_embs=c["cp_embs"], cols=H, out=P.guarded(n * H))
    what = f"k_assemble_rows H={H}"
    _guards_intact(out, what)
    got = P.payload(out).reshape(n, H)
    want = P.assemble_reference(c)
    for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS):
        _equal(got[i], want[i], f"{what} row {i} (text_row {tr}, codec_id {cid})")
    none = [i for i, (tr, cid) in enumerate(P.ASSEMBLE_ROWS) if tr < 0 and cid == -1]
    assert all((got[i].view(np.uint32) == 0).all() for i in none), f"{what}: no text row and no codec part must give +0.0"


@pytest.mark.parametrize("cols", P.WIDTHS)
@pytest.mark.parametrize("rows", [1, 3])
def test_copy_rows(rows, cols):
    src, ldd = P.copy_case(rows, cols)
    assert src.shape[1] != ldd
    out = q.prompt_rows_ex(ROWS_COPY, src=src, cols=cols, ldd=ldd, out=P.guarded(rows * ldd))
    what = f"k_copy_rows rows={rows} cols={cols} lds={src.shape[1]} ldd={ldd}"
    _guards_intact(out, what)
    _equal(P.payload(out).reshape(rows, ldd), P.copy_reference(src, cols, ldd), what)          # the padding beyond cols keeps the sentinel


@pytest.mark.parametrize("cols", P.WIDTHS)
def test_scatter_rows(cols):
    src = P.scatter_case(cols)
    out = q.prompt_rows_ex(ROWS_SCATTER, src=src, dst_row=P.SCATTER_DST, cols=cols, n_rows=P.SCATTER_ROWS, out=P.guarded(P.SCATTER_ROWS * cols))
    what = f"k_scatter_rows cols={cols}"
    _guards_intact(out, what)
    _equal(P.payload(out).reshape(P.SCATTER_ROWS, cols), P.scatter_reference(src, cols), what)  # every row not named keeps the sentinel


@pytest.mark.parametrize("n", P.PUBLISH_N)
def test_publish_text(n):
    ent = P.publish_case(n)
    arrs = [P.guarded(P.PUBLISH_ROWS, np.int32) for _ in range(3)]
    q.prompt_rows_ex(ROWS_PUBLISH, ent=ent, n_rows=P.PUBLISH_ROWS, trail_len=arrs[0], text_ready=arrs[1], limit=arrs[2])
    for name, got, want in zip(("trail_len", "text_ready", "limit"), arrs, P.publish_reference(ent)):
        what = f"k_publish_text n={n} {name}"
        _guards_intact(got, what)
        _equal(P.payload(got), want, what)
