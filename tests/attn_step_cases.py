"""Cases, float64 reference and frozen constants of the decode-attention form tests (test_gpu_attention_forms.py on the GPU,
test_attention_forms_reference.py on the CPU). TEST INFRASTRUCTURE.

One step of decode attention as q3_attn_step_ex runs it: q|k|v of a row (from the row itself, from K-slice sums, or from the table
row a folded gather picks), per-head q/k RMSNorm, rotate-half RoPE at the row's position, append, GQA attention over the cache
and the step's own rows. The reference is np_reference.rms_norm / rotate_half in float64, as in test_gpu_attention_op.py.

Tolerance (that file's rule). D_REF / D_REF_K are the worst deviation of THIS reference run in numpy float32 from float64 over
all_cases(), relative to the case's max: D_REF for `out`, D_REF_K for an appended row that is computed (the K row; the V row of a
slice-sum case, a sum of slices over a square root). A kernel gets 4 x: a factor of two for another summation order, another for
a fast exp. The CPU file re-measures them."""
import functools

import numpy as np

from np_reference import rms_norm, rotate_half, rope_cos_sin

EPS = 1e-6
HD = 128
PAGE = 128
SLAB_SLOTS = 32
RATIOS = [(2, 2), (4, 2), (4, 1)]               # heads / kv heads = 1, 2, 4
HOT = 5.3                                         # logit of an aligned key = 128^-0.5 * HOT * |q|^2 ~ 60 with |q|^2 ~ 128
EDGE_POS = (126, 127, 128, 129, 255, 256, 383)    # last rows of a page, first rows of the next, in one 7-row call
EDGE_SPLITS = (1, 3, 16, 64)

# measured by measure_d_ref() on the CPU (numpy float32 against float64 over all_cases()); test_attention_forms_reference.py
# asserts 0.5 * C <= measured <= C for each. Measured: 1.53e-6 for `out` (the worst cases are the 1024- and 1280-position ones, whose
# outputs — averages over a thousand random rows — are small against the float32 sums behind them; the 8192-key case gives 5.7e-7
# and needs no constant of its own), 1.96e-7 for the appended rows. The GPU bounds are therefore 6.4e-6 and 8.4e-7.
D_REF = 1.6e-6
D_REF_K = 2.1e-7
assert 4 * D_REF <= 2e-5                          # a looser figure would mean the inputs are ill-conditioned


# ---------------------------------------------------------------- bf16
def bf16_rne_bits(x):
    """f32 array -> uint16 bf16 bits, round to nearest even (finite inputs)"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_to_f32(bits):
    return (np.asarray(bits, dtype=np.uint16).astype(np.uint32) << 16).view(np.float32)


def bf16_round(x):
    return bf16_to_f32(bf16_rne_bits(x))


def bf16_rne_of_f64(x):
    """float64 array -> (nearest bf16 value as float64, ties to even; spacing of bf16 numbers at x). Normal range only."""
    x = np.asarray(x, dtype=np.float64)
    _, e = np.frexp(np.where(x == 0, 1.0, x))
    ulp = np.ldexp(1.0, e - 8)                    # 8 significant bits: |x| / ulp in [128, 256)
    return np.rint(x / ulp) * ulp, ulp            # np.rint rounds halves to even


# exact ties of the bf16 rounding: 1 + 2^-8 lies midway between 1 (even) and 1 + 2^-7, 1 + 3 * 2^-8 midway between 1 + 2^-7 (odd)
# and 1 + 2^-6 — a truncating store gets the second wrong, a round-half-up store the first
TIES = np.array([s * m * 2.0 ** e for e in (-3, 0, 2, 5) for m in (1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8) for s in (1.0, -1.0)], dtype=np.float32)
TIES_RNE = np.array([s * m * 2.0 ** e for e in (-3, 0, 2, 5) for m in (1.0, 1 + 2.0 ** -6) for s in (1.0, -1.0)], dtype=np.float32)


# ---------------------------------------------------------------- pages
def page_slots(n_seq, n_pg, n_slabs, seed):
    """[n_seq][n_pg] distinct slots of 0 .. 32 * n_slabs - 1. The slots are cut into n_pg bands; the pages of a sequence take
    the same place in every band (so two of them are a whole number of bands apart: never neighbours while a band is wider than
    one slot) in an order drawn per sequence, and every sequence has a place of its own."""
    total = SLAB_SLOTS * n_slabs
    band = total // n_pg
    assert band >= 1 and n_seq <= band, "not enough slots"
    rng = np.random.default_rng(seed)
    place = rng.permutation(band)[:n_seq]
    out = np.zeros((n_seq, n_pg), dtype=np.int32)
    for s in range(n_seq):
        order = rng.permutation(n_pg)
        if n_pg > 2 and (np.diff(order) > 0).all():
            order = order[::-1]
        out[s] = order * band + place[s]
    return out


def scatter_model(logical, slots, rot, n_slots):
    """numpy model of the entry's scatter: logical [n_seq][nkv][max_seq][128] -> pages [n_slots][nkv][128][128]; position p of
    (sequence, kv head) sits in row (p + rot[seq][page][head]) % 128 of page slots[seq][p // 128]"""
    n_seq, nkv, max_seq, _ = logical.shape
    pages = np.full((n_slots, nkv, PAGE, HD), np.nan, dtype=logical.dtype)
    for s in range(n_seq):
        for g in range(nkv):
            for p in range(max_seq):
                pages[slots[s, p // PAGE], g, (p + rot[s, p // PAGE, g]) % PAGE] = logical[s, g, p]
    return pages


def gather_model(pages, slots, rot, max_seq):
    n_seq, nkv = slots.shape[0], pages.shape[1]
    out = np.zeros((n_seq, nkv, max_seq, HD), dtype=pages.dtype)
    for s in range(n_seq):
        for g in range(nkv):
            for p in range(max_seq):
                out[s, g, p] = pages[slots[s, p // PAGE], g, (p + rot[s, p // PAGE, g]) % PAGE]
    return out


def pairs_across_pages(pos, n_splits):
    """the key pairs (pe, pe + 1) that the two 32-lane groups of a wave of the one-launch kernel ask for together and that lie in
    different pages: split s covers [s * chunk, ...) with chunk = ceil((pos + 1) / n_splits), its waves take (start + 2 m,
    start + 2 m + 1) — so a pair straddles a page edge only where a split starts on an odd position"""
    n = pos + 1
    chunk = -(-n // n_splits)
    out = []
    for s in range(n_splits):
        start, end = s * chunk, min(s * chunk + chunk, n)
        out += [(pe, pe + 1) for pe in range(start, end - 1, 2) if pe // PAGE != (pe + 1) // PAGE]
    return out


# ---------------------------------------------------------------- cases
@functools.lru_cache(maxsize=None)
def rope(max_seq):
    c, s = rope_cos_sin(1.0e6, HD, np.arange(max_seq))
    return c.astype(np.float32), s.astype(np.float32)


def norm_rope(x, w, pos, max_seq, dtype):
    """x [B][heads][128] -> per-head RMSNorm * w, rotate-half RoPE at pos[b]"""
    c, s = rope(max_seq)
    c = c.astype(dtype)[pos][:, None, :]; s = s.astype(dtype)[pos][:, None, :]
    return rotate_half(rms_norm(x.astype(dtype), w.astype(dtype), dtype(EPS)), c, s)


def row_positions(c):
    rps = c["rps"]
    return np.repeat(c["pos"], rps) + np.tile(np.arange(rps, dtype=np.int32), len(c["pos"]))


def gather_logits(B, vocab, rng):
    """rows designed for the argmax: the maximum at index 0, at vocab - 1, duplicated at (5, 1029) and at (1029, 2043) — the
    lower index must win —, an all-equal row (0 wins), a row that is -inf but for one entry; then plain random rows"""
    lg = rng.standard_normal((B, vocab)).astype(np.float32)
    cl = lambda i: min(i, vocab - 1)
    top = np.float32(9.0)
    designs = [lambda r: r.__setitem__(0, top), lambda r: r.__setitem__(vocab - 1, top),
               lambda r: (r.__setitem__(cl(5), top), r.__setitem__(cl(1029), top)),
               lambda r: (r.__setitem__(cl(1029) if vocab > 3 else 1, top), r.__setitem__(cl(2043), top)),
               lambda r: r.fill(np.float32(0.25)),
               lambda r: (r.fill(-np.inf), r.__setitem__(cl(777), np.float32(-3.0)))]
    for b, d in enumerate(designs[:B]):
        d(lg[b])
    return lg


@functools.lru_cache(maxsize=None)
def make_case(nh, nkv, max_seq, pos, rps=1, kind="plain", hot=None, S=0, vocab=0, seed=0):
    """inputs of one step (read-only, shared by the variants, layouts and split counts that run it).
    kind: "plain"; "bf16" (cache exact in bf16, ties in v); "slices" (q|k|v as S slice sums over K = 1024); "gather" (g_logits
    over `vocab`); "tok" (variant 3 with g_tok). hot: positions of the softmax-stress key, one per row."""
    n_seq = len(pos); B = n_seq * rps; nrep = nh // nkv; ld = (nh + 2 * nkv) * HD
    rng = np.random.default_rng([nh, nkv, max_seq, rps, S, vocab, seed, sum(pos), len(kind)] + list(pos[:8]))
    c = dict(nh=nh, nkv=nkv, max_seq=max_seq, rps=rps, B=B, kind=kind, pos=np.array(pos, dtype=np.int32))
    qkv = rng.standard_normal((B, ld)).astype(np.float32)
    qw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kc = rng.standard_normal((n_seq, nkv, max_seq, HD)).astype(np.float32)
    vc = rng.standard_normal((n_seq, nkv, max_seq, HD)).astype(np.float32)
    if kind == "bf16":
        kc = bf16_round(kc); vc = bf16_round(vc)
        v = qkv[:, (nh + nkv) * HD:]                         # (a view: the ties go into qkv)
        v[:, :len(TIES)] = TIES
        v[:, HD - len(TIES):HD] = TIES[::-1]
    if hot is not None:
        # one key per row ~60 logits above the rest for the first q head of every kv head (test_gpu_attention_op.py's stress case)
        assert rps == 1 and kind == "plain" and all(h < p for h, p in zip(hot, pos))
        kw = (HOT * np.ones(HD)).astype(np.float32); qw = np.ones(HD, dtype=np.float32)
        qr = norm_rope(qkv[:, :nh * HD].reshape(B, nh, HD), qw, c["pos"], max_seq, np.float64)
        for b in range(B):
            for g in range(nkv):
                kc[b, g, hot[b]] = (HOT * qr[b, g * nrep]).astype(np.float32)
        c["hot"] = tuple(hot)
    if kind == "slices":
        # the split-K GEMM's slice sums: S partial rows that add up to about the usual q|k|v before the norm's division
        part = (rng.standard_normal((S, B, ld)) * (4.0 / np.sqrt(S))).astype(np.float32)
        ssq = (1024.0 / S * (12.0 + 8.0 * rng.random((S, B)))).astype(np.float32)
        c.update(qkv_part=part, qkv_ssq=ssq, qkv_K=1024, qkv_eps=EPS)
        qkv = None
    if kind in ("gather", "tok"):
        V = vocab
        c["g_qkv_tab"] = rng.standard_normal((V, ld)).astype(np.float32)
        c["g_proj_dim"] = 200; c["g_ldx"] = 208
        c["g_proj_tab"] = rng.standard_normal((V, 200)).astype(np.float32)
        c["g_x"] = np.full((n_seq if kind == "tok" else B, 208), -7.5, dtype=np.float32)
        if kind == "gather":
            c["g_logits"] = gather_logits(B, V, rng)
            c["g_max_frames"] = 3; c["g_code_slot"] = 1 + (nh + V) % 15
            fi = (np.arange(B) % 3).astype(np.int32); fi[-1] = 3          # the last row's frame is beyond the table: no code
            c["g_frame_idx"] = fi
            c["g_codes"] = (0xabc00000 + np.arange(B * 3 * 16, dtype=np.uint32)).reshape(B, 3, 16)
            qkv = None
        else:
            c["g_tok"] = rng.integers(0, V, n_seq).astype(np.uint32)
    c.update(qkv=qkv, qw=qw, kw=kw, kc=kc, vc=vc)
    for a in c.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return c


def effective_qkv(c, dtype):
    """the q|k|v rows the step works on, [B][(nh + 2 nkv) * 128] in `dtype`"""
    if c.get("qkv_part") is not None:
        part, ssq = c["qkv_part"], c["qkv_ssq"]
        s = np.zeros(part.shape[1:], dtype=dtype); tot = np.zeros(part.shape[1], dtype=dtype)
        for i in range(part.shape[0]):                       # ascending slice order
            s = s + part[i].astype(dtype); tot = tot + ssq[i].astype(dtype)
        return s / np.sqrt(tot / dtype(c["qkv_K"]) + dtype(c["qkv_eps"]))[:, None]
    if c.get("g_logits") is not None:
        return c["g_qkv_tab"][np.argmax(c["g_logits"], axis=1)].astype(dtype)      # np.argmax: the first maximum
    x = c["qkv"].astype(dtype)
    if c.get("g_tok") is not None:
        x[1::2] = c["g_qkv_tab"][c["g_tok"]].astype(dtype)
    return x


def reference(c, dtype=np.float64, k_rows=None, v_rows=None):
    """(out [B][nh*128], appended K rows [B][nkv][128], appended V rows [B][nkv][128]) in `dtype` arithmetic. k_rows / v_rows:
    attend over THESE appended rows instead of the computed ones (a cache as it stands after a step that rounded them)."""
    nh, nkv, rps, B, max_seq = c["nh"], c["nkv"], c["rps"], c["B"], c["max_seq"]
    nrep = nh // nkv
    x = effective_qkv(c, dtype)
    rp = row_positions(c)
    qr = norm_rope(x[:, :nh * HD].reshape(B, nh, HD), c["qw"], rp, max_seq, dtype)
    kr = norm_rope(x[:, nh * HD:(nh + nkv) * HD].reshape(B, nkv, HD), c["kw"], rp, max_seq, dtype)
    v = x[:, (nh + nkv) * HD:].reshape(B, nkv, HD)
    ka = kr if k_rows is None else np.asarray(k_rows).astype(dtype)
    va = v if v_rows is None else np.asarray(v_rows).astype(dtype)
    out = np.zeros((B, nh, HD), dtype=dtype)
    scale = dtype(HD ** -0.5)
    for b in range(B):
        s, r = divmod(b, rps); base = int(c["pos"][s])
        for g in range(nkv):
            K = np.concatenate([c["kc"][s, g, :base].astype(dtype), ka[s * rps:s * rps + r + 1, g]], 0)
            V = np.concatenate([c["vc"][s, g, :base].astype(dtype), va[s * rps:s * rps + r + 1, g]], 0)
            sc = (qr[b, g * nrep:(g + 1) * nrep] @ K.T) * scale                   # [nrep][keys]
            pr = np.exp(sc - sc.max(1, keepdims=True)); pr = pr / pr.sum(1, keepdims=True)
            out[b, g * nrep:(g + 1) * nrep] = pr @ V
    return out.reshape(B, nh * HD), kr, v


def reference_loops(c):
    """the same in plain float64 loops, key by key (small cases: the check of the vectorised form)"""
    nh, nkv, rps, B = c["nh"], c["nkv"], c["rps"], c["B"]
    nrep = nh // nkv
    x = effective_qkv(c, np.float64)
    cs, sn = rope(c["max_seq"])
    rp = row_positions(c)

    def nr(vec, w, p):
        y = vec / np.sqrt(np.mean(vec * vec) + EPS) * w.astype(np.float64)
        o = np.zeros(HD)
        for i in range(64):
            co, si = float(cs[p, i]), float(sn[p, i])
            o[i] = y[i] * co - y[i + 64] * si
            o[i + 64] = y[i + 64] * co + y[i] * si
        return o
    kr = np.array([[nr(x[b, (nh + g) * HD:(nh + g + 1) * HD], c["kw"], rp[b]) for g in range(nkv)] for b in range(B)])
    v = x[:, (nh + nkv) * HD:].reshape(B, nkv, HD)
    out = np.zeros((B, nh, HD))
    for b in range(B):
        s, r = divmod(b, rps); base = int(c["pos"][s])
        for h in range(nh):
            g = h // nrep
            q = nr(x[b, h * HD:(h + 1) * HD], c["qw"], rp[b])
            keys = [c["kc"][s, g, p].astype(np.float64) for p in range(base)] + [kr[s * rps + i, g] for i in range(r + 1)]
            vals = [c["vc"][s, g, p].astype(np.float64) for p in range(base)] + [v[s * rps + i, g] for i in range(r + 1)]
            sc = [float(np.dot(q, k)) / np.sqrt(128.0) for k in keys]
            m = max(sc); w = [np.exp(t - m) for t in sc]; tot = sum(w)
            for wi, vi in zip(w, vals):
                out[b, h] += wi / tot * vi
    return out.reshape(B, nh * HD), kr, v


@functools.lru_cache(maxsize=None)
def ref64(key):
    return reference(make_case(*key))


# ---------------------------------------------------------------- the case tables (make_case keys)
def K(nh, nkv, max_seq, pos, rps=1, kind="plain", hot=None, S=0, vocab=0, seed=0):
    return (nh, nkv, max_seq, tuple(pos), rps, kind, hot, S, vocab, seed)


def edge_keys(kind="plain"):
    return [K(nh, nkv, 512, EDGE_POS, kind=kind) for nh, nkv in RATIOS]


def deep_keys():
    """the last row of the scalar table form (8 pages), rows of a 10-page table, and the last position a table can name"""
    return ([K(nh, nkv, 1024, (1023, 896)) for nh, nkv in RATIOS] + [K(nh, nkv, 1280, (1030, 1151, 1152)) for nh, nkv in RATIOS] +
            [K(4, 2, 8192, (8191,))])


def hot_keys():
    return [K(nh, nkv, 256, (200, 200), hot=(127, 128)) for nh, nkv in RATIOS]


def multirow_keys():
    return [K(nh, nkv, 256, (0, 126), rps=rps) for nh, nkv in RATIOS for rps in (2, 5)]


def first2_keys(kind="plain"):
    return [K(nh, nkv, 17, (0,) * n, rps=2, kind=kind, vocab=64 if kind == "tok" else 0) for nh, nkv in RATIOS for n in (1, 8)]


GATHER_VOCABS = (2048, 2044, 2047, 3)
GATHER_POS_FUSED = (0, 1, 5, 15, 16, 3, 9)          # variant 0: a 17-position cache, one position per row
GATHER_POS_CP = (1, 4, 8, 15)                       # variant 2: NK = 4, 8, 16, 16


def gather_keys(variant):
    ks = []
    for vocab in GATHER_VOCABS:
        for nh, nkv in (RATIOS if vocab == 2048 else [(4, 2)]):
            if variant == 0:
                ks.append(K(nh, nkv, 17, GATHER_POS_FUSED, kind="gather", vocab=vocab))
            else:
                ks += [K(nh, nkv, 17, (p,) * 7, kind="gather", vocab=vocab) for p in GATHER_POS_CP]
    return ks


def slice_keys(variant, paged=False):
    ks = []
    for B in (17, 64):
        for S in (1, 2, 8):
            for nh, nkv in (RATIOS if (B, S) == (17, 2) else [(4, 2)]):
                if variant == 2:
                    ks.append(K(nh, nkv, 17, (7,) * B, kind="slices", S=S))
                else:
                    ms = 128 if paged else 256                # paged: one page per sequence, 64 sequences fill two slabs
                    pos = tuple(int(v) for v in np.random.default_rng(B * 10 + S).integers(0, ms, B))
                    ks.append(K(nh, nkv, ms, pos, kind="slices", S=S))
    return ks


def zero_keys():
    return [K(4, 2, 256, (3, 130, 255)), K(4, 2, 17, (7,) * 5), K(4, 2, 17, (0,) * 3, rps=2)]      # for variants 0, 2, 3


def all_cases():
    ks = (edge_keys() + edge_keys("bf16") + deep_keys() + hot_keys() + multirow_keys() + first2_keys() + first2_keys("tok") +
          gather_keys(0) + gather_keys(2) + slice_keys(0) + slice_keys(0, True) + slice_keys(2) + zero_keys())
    seen, out = set(), []
    for k in ks:
        if k not in seen:
            seen.add(k); out.append(k)
    return out


def measure_d_ref(keys=None):
    """worst deviation of float32 numpy from float64 over the cases: (out, computed appended rows), relative to the case's max"""
    d = dk = 0.0
    for key in (all_cases() if keys is None else keys):
        c = make_case(*key)
        o64, k64, v64 = ref64(key)
        o32, k32, v32 = reference(c, np.float32)
        d = max(d, float(np.abs(o32 - o64).max() / np.abs(o64).max()))
        dk = max(dk, float(np.abs(k32 - k64).max() / np.abs(k64).max()))
        if c["kind"] == "slices":
            dk = max(dk, float(np.abs(v32 - v64).max() / np.abs(v64).max()))
    return d, dk
