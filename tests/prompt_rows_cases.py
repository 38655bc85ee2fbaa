"""Inputs, tables and bit-exact references of the prompt-row kernel tests (test_gpu_prompt_rows.py on the GPU,
test_prompt_rows_reference.py on the CPU). TEST INFRASTRUCTURE — no test lives here.

The kernels (q3_kernels_lm.hip) move rows and add at most two float32 values per element, so every reference is exact: the GPU
file compares bits, not deviations.
  k_gather_rows_bf16   out[r] = f32(table[ids[r]])                          (bf16 -> f32 is a 16-bit shift)
  k_assemble_rows      out[i] = text part + codec part, by (text_row, codec_id): text_row >= 0 -> rows[text_row]; codec_id >= 0 ->
                       codec_emb[codec_id], -1 -> nothing, -2 -> xvec, <= -3 -> ICL reference frame f = -3 - codec_id:
                       codec_emb[c0] + e0[c1] + ... + e14[c15], added left to right, every add rounded to float32
  k_copy_rows          dst[r][:cols] = src[r][:cols] with lds != ldd
  k_scatter_rows       rows[dst_row[r]] = src[r] where dst_row[r] >= 0
  k_publish_text       (trail_len, text_ready, limit)[b] = entry's three values"""
import functools

import numpy as np

GUARD = 64
WIDTHS = (8, 255, 256, 257, 1024)        # the edges of the 256-thread stride loop: one partial pass, 255 / 256 / 257, four whole passes
SENT = np.float32(-7.0625e33)            # sentinel in every destination: no kernel computes this value
SENT_I = np.int32(-0x5a5a5a5b)

VOCAB = 37                               # rows of the bf16 tables
CP_VOCAB = 29
N_TEXT = 6                               # rows of `rows`
N_REF = 5                                # ICL reference frames


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def _bf16_table(rng, shape):
    """finite bf16 bits over ~20 binades: sums of such values round in float32, so the order of a chain shows in its bits"""
    x = rng.standard_normal(shape) * np.exp2(rng.integers(-10, 11, size=shape))
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def guarded(payload_elems, dtype=np.float32):
    """a flat destination: GUARD sentinels, the payload (sentinels too), GUARD sentinels"""
    return np.full(payload_elems + 2 * GUARD, SENT if dtype == np.float32 else SENT_I, dtype=dtype)


def payload(buf):
    return buf[GUARD:buf.size - GUARD]


def same_bits(a, b):
    a = np.ascontiguousarray(a); b = np.ascontiguousarray(b)
    return a.shape == b.shape and (a.view(np.uint32) == b.view(np.uint32)).all()


def first_diff(a, b):
    d = np.argwhere(np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32))
    return None if len(d) == 0 else tuple(int(i) for i in d[0])


# ---------------------------------------------------------------- gather
@functools.lru_cache(maxsize=None)
def gather_case(n, dim):
    """ids repeat and name the first and the last table row"""
    rng = np.random.default_rng(1000 + n * 7 + dim)
    table = _bf16_table(rng, (VOCAB, dim))
    ids = np.array([VOCAB - 1] if n == 1 else [0, VOCAB - 1, 5, 0, VOCAB - 1][:n], dtype=np.uint32)
    assert ids.size == n
    table.setflags(write=False); ids.setflags(write=False)
    return table, ids


def gather_reference(table, ids):
    return bf16_to_f32(table[ids])


# ---------------------------------------------------------------- assemble
# one launch covers every (text_row, codec_id) combination: a text row or none, with a codec id (first / last table row), -1, -2,
# the first ICL frame (-3) and the last one (-3 - (N_REF - 1))
ASSEMBLE_ROWS = [(tr, cid) for tr in (0, N_TEXT - 1, -1) for cid in (0, VOCAB - 1, -1, -2, -3, -3 - (N_REF - 1))] + [(2, -4), (-5, 7)]


@functools.lru_cache(maxsize=None)
def assemble_case(H):
    rng = np.random.default_rng(2000 + H)
    c = dict(H=H,
             rows=(rng.standard_normal((N_TEXT, H)) * np.exp2(rng.integers(-8, 9, size=(N_TEXT, H)))).astype(np.float32),
             codec_emb=_bf16_table(rng, (VOCAB, H)), xvec=rng.standard_normal(H).astype(np.float32),
             cp_embs=_bf16_table(rng, (15, CP_VOCAB, H)),
             text_row=np.array([r[0] for r in ASSEMBLE_ROWS], dtype=np.int32), codec_id=np.array([r[1] for r in ASSEMBLE_ROWS], dtype=np.int32))
    ref = np.empty((N_REF, 16), dtype=np.uint32)
    ref[:, 0] = rng.integers(0, VOCAB, size=N_REF); ref[:, 1:] = rng.integers(0, CP_VOCAB, size=(N_REF, 15))
    ref[0, 0] = VOCAB - 1; ref[0, 1] = CP_VOCAB - 1; ref[N_REF - 1, 15] = CP_VOCAB - 1; ref[N_REF - 1, 0] = 0      # the tables' last and first rows
    c["ref_codes"] = ref
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


def icl_terms(c, frame):
    """the 16 float32 rows an ICL reference frame adds up, in the kernel's order"""
    fr = c["ref_codes"][frame]
    return [bf16_to_f32(c["codec_emb"][fr[0]])] + [bf16_to_f32(c["cp_embs"][g - 1][fr[g]]) for g in range(1, 16)]


def chain_left(terms):
    acc = terms[0].astype(np.float32)
    for t in terms[1:]:
        acc = (acc + t).astype(np.float32)          # float32 + float32 in numpy: one rounded add
    return acc


def chain_right(terms):
    acc = terms[-1].astype(np.float32)
    for t in terms[-2::-1]:
        acc = (t + acc).astype(np.float32)
    return acc


def chain_pairwise(terms):
    t = [x.astype(np.float32) for x in terms]
    while len(t) > 1:
        t = [(t[i] + t[i + 1]).astype(np.float32) for i in range(0, len(t), 2)]
    return t[0]


def assemble_reference(c, chain=chain_left):
    H = c["H"]
    out = np.zeros((len(c["text_row"]), H), dtype=np.float32)
    for i, (tr, cid) in enumerate(zip(c["text_row"].tolist(), c["codec_id"].tolist())):
        if cid >= 0:
            cv = bf16_to_f32(c["codec_emb"][cid])
        elif cid == -2:
            cv = c["xvec"]
        elif cid <= -3:
            cv = chain(icl_terms(c, -3 - cid))
        else:
            cv = None
        if tr >= 0 and cv is not None:
            out[i] = (c["rows"][tr] + cv).astype(np.float32)
        elif tr >= 0:
            out[i] = c["rows"][tr]
        elif cv is not None:
            out[i] = cv
        # neither: +0.0
    return out


# ---------------------------------------------------------------- copy
@functools.lru_cache(maxsize=None)
def copy_case(rows, cols):
    rng = np.random.default_rng(3000 + rows * 11 + cols)
    src = rng.standard_normal((rows, cols + 3)).astype(np.float32)          # lds = cols + 3, ldd = cols + 5
    src.setflags(write=False)
    return src, cols + 5


def copy_reference(src, cols, ldd):
    want = np.full((src.shape[0], ldd), SENT, dtype=np.float32)
    want[:, :cols] = src[:, :cols]
    return want


# ---------------------------------------------------------------- scatter
SCATTER_ROWS = 11
SCATTER_DST = np.array([10, -1, 3, 0, -1, 7, -1, 5], dtype=np.int32)      # in no order; the first and the last row of `rows`; three padding rows


@functools.lru_cache(maxsize=None)
def scatter_case(cols):
    rng = np.random.default_rng(4000 + cols)
    src = rng.standard_normal((SCATTER_DST.size, cols)).astype(np.float32)
    src.setflags(write=False)
    return src


def scatter_reference(src, cols):
    want = np.full((SCATTER_ROWS, cols), SENT, dtype=np.float32)
    for r, d in enumerate(SCATTER_DST.tolist()):
        if d >= 0:
            want[d] = src[r]
    return want


# ---------------------------------------------------------------- publish
PUBLISH_ROWS = 80
PUBLISH_N = (1, 64, 65)                  # one lane; a whole workgroup of 64; one entry into a second workgroup


@functools.lru_cache(maxsize=None)
def publish_case(n):
    rng = np.random.default_rng(5000 + n)
    b = np.array([PUBLISH_ROWS - 1]) if n == 1 else \
        np.concatenate([[PUBLISH_ROWS - 1], 1 + rng.permutation(PUBLISH_ROWS - 2)[:n - 2], [0]])      # the first entry names the last row, the last row 0
    assert len(set(b.tolist())) == n == b.size
    ent = np.empty((n, 4), dtype=np.int32)
    ent[:, 0] = b; ent[:, 1:] = rng.integers(1, 1 << 20, size=(n, 3))
    ent.setflags(write=False)
    return ent


def publish_reference(ent):
    want = [np.full(PUBLISH_ROWS, SENT_I, dtype=np.int32) for _ in range(3)]
    for (b, tl, tr, lim) in ent.tolist():
        want[0][b], want[1][b], want[2][b] = tl, tr, lim
    return want
