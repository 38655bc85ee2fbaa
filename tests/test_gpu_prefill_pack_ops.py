"""Op-level tests of the PACKED prefill attention launches (-m gpu): q3_attn_prefill_packed_ex runs the packed
k_qknorm_rope_kv, the packed k_kv_planes and one packed launch of k_attn_prefill_t / k_attn_prefill_x3 per kernel present over
sequences of unequal length laid end to end (cases: prefill_pack_cases.py; GQA ratios 2 and 1, two slabs of pages, one contiguous
case per kernel).

Per case:
  1. every sequence's rows of `out` and its K / V cache over [0, len) are BIT-EQUAL to q3_attn_prefill_ex on that sequence alone
     (n_seq = 1, rps = len, base_pos = 0, the same kernel, the same inputs) — the contract of the packed pass, no tolerance;
  2. `out` against float64 (attn_reference of prefill_ops_cases.py per sequence) within 4 * D_REF, the appended K rows within
     4 * D_REF_K: the bounds tests/test_gpu_prefill_paged.py holds these kernels to;
  3. the sentinel columns of `out`, the NaN fill of the plane buffer behind the last sequence's tiles, every cache position >= len
     and the slabs outside the cache rows (stray) are untouched;
  4. the same sequences packed in another order give every sequence the same bits."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import prefill_ops_cases as C
import prefill_pack_cases as P
from prefill_ops_cases import GEN_T, X3, HD, EPS, SENT, D_REF, D_REF_K

pytestmark = pytest.mark.gpu

assert [k for k in os.environ if k.startswith("Q3_PREFILL_ATTN_") or k.startswith("Q3_GEMM_") or k == "Q3_KV_CONTIGUOUS"] == [], \
    "prefill / KV layout knobs set: the cases would not reach the kernels and the layout they name"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_diff(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    return None if len(d) == 0 else tuple(int(i) for i in d[0])


def _run_pack(p, kernel, layout, slots):
    rc, rs = C.rope(p["max_seq"])
    out_in = np.full((int(sum(p["lens"])), p["nh"] * HD + 4), SENT, dtype=np.float32)
    kw = dict(kernel=kernel, out=out_in)
    if layout:
        kw.update(layout=1, n_layers=2, layer=1, n_slabs=2, page_slots=slots)
    return q.attn_prefill_packed_ex(p["qkv"], p["lens"], p["qw"], p["kw"], EPS, rc, rs, p["kc"], p["vc"], p["nh"], p["nkv"], **kw)


def _run_solo(p, i, kernel, layout, slots):
    c = P.seq_case(p, i)
    rc, rs = C.rope(c["max_seq"])
    out_in = np.full((c["rps"], c["nh"] * HD + 4), SENT, dtype=np.float32)
    kw = dict(kernel=P.kernel_of(kernel, c["rps"]), halves=1, out=out_in)
    if layout:
        kw.update(layout=1, n_layers=2, layer=1, n_slabs=2, page_slots=slots[i:i + 1])
    return q.attn_prefill_ex(c["qkv"], 1, 0, c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], c["nh"], c["nkv"], **kw)


@pytest.mark.parametrize("ratio", P.RATIOS, ids=lambda r: f"nh{r[0]}-nkv{r[1]}")
@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c[0])
def test_packed_prefill_attention(case, ratio):
    name, lens, kernel, layout = case
    nh, nkv = ratio
    p = P.pack_case(nh, nkv, lens)
    slots = P.pack_slots(p) if layout else None
    what = f"{name} nh{nh} nkv{nkv}"
    out, kc, vc, path, info = _run_pack(p, kernel, layout, slots)
    kinds = {P.kernel_of(kernel, L) for L in lens}
    assert path == (int(GEN_T in kinds), int(X3 in kinds)), f"{what}: launches {path}"
    # 3. stray writes first: they name a fault most directly
    assert info["stray"] == 0, f"{what}: {info['stray']} slab elements outside the cache rows changed, the first at offset {info['stray_at']}"
    rows = int(sum(lens))
    assert (_bits(out[:, nh * HD:]) == _bits(np.full((rows, 4), SENT))).all(), f"{what}: out written beyond nh * 128 columns"
    if X3 in kinds:
        still, size = info["plane_tail"]
        assert size > 0 and still == size, f"{what}: {size - still} bytes of the plane buffer behind the last sequence's tiles were written"
    out = out[:, :nh * HD]
    assert np.isfinite(out).all(), f"{what}: non-finite outputs (a row of another sequence or a NaN plane read in)"
    for i, L in enumerate(lens):
        r0 = int(p["row0"][i]); w = f"{what} sequence {i} ({L} rows from row {r0})"
        for nm, got, want in (("K", kc, p["kc"]), ("V", vc, p["vc"])):
            assert _first_diff(got[i, :, L:], want[i, :, L:]) is None, f"{w}: {nm} cache changed at positions >= {L}, first at (kv head, pos - len, d) {_first_diff(got[i, :, L:], want[i, :, L:])}"
        # 1. the contract: the bits of the sequence's own launch
        solo = _run_solo(p, i, kernel, layout, slots)
        o1, k1, v1, path1 = solo[0], solo[1], solo[2], solo[3]
        assert path1 == (P.kernel_of(kernel, L), 1), f"{w}: the solo launch ran {path1}"
        assert _first_diff(out[r0:r0 + L], o1[:, :nh * HD]) is None, f"{w}: out differs from the sequence's own launch, first at (row, col) {_first_diff(out[r0:r0 + L], o1[:, :nh * HD])}"
        for nm, a, b in (("K", kc[i, :, :L], k1[0, :, :L]), ("V", vc[i, :, :L], v1[0, :, :L])):
            assert _first_diff(a, b) is None, f"{w}: {nm} cache over [0, {L}) differs from the sequence's own launch, first at (kv head, pos, d) {_first_diff(a, b)}"
        # 2. float64
        o64, k64 = C.attn_reference(P.seq_case(p, i))
        dev = float(np.abs(out[r0:r0 + L] - o64).max() / np.abs(o64).max())
        k_new = kc[i, :, :L].transpose(1, 0, 2)
        dev_k = float(np.abs(k_new - k64).max() / np.abs(k64).max())
        print(f"{w}: out dev {dev:.3e} = {dev / D_REF:.2f} D_REF (bound 4), K row dev {dev_k:.3e} = {dev_k / D_REF_K:.2f} D_REF_K (bound 4)")
        assert dev <= 4 * D_REF, f"{w}: out deviates {dev:.3e} > {4 * D_REF:.3e} from float64"
        assert dev_k <= 4 * D_REF_K, f"{w}: appended K rows deviate {dev_k:.3e} > {4 * D_REF_K:.3e} from float64"
        v_in = p["qkv"][r0:r0 + L, (nh + nkv) * HD:].reshape(L, nkv, HD).transpose(1, 0, 2)
        assert _first_diff(vc[i, :, :L], v_in) is None, f"{w}: appended V rows are not the v part of qkv"
    # 4. another pack order: the last sequence first, the rest rotated by two
    n = len(lens)
    order = [n - 1] + [(j + 2) % (n - 1) for j in range(n - 1)]
    assert sorted(order) == list(range(n)) and order != list(range(n))
    pp = P.permuted(p, order)
    out2, kc2, vc2, _, info2 = _run_pack(pp, kernel, layout, slots)
    assert info2["stray"] == 0, f"{what} (permuted): stray writes, the first at offset {info2['stray_at']}"
    for j, i in enumerate(order):
        L = lens[i]; a0 = int(p["row0"][i]); b0 = int(pp["row0"][j])
        assert _first_diff(out[a0:a0 + L], out2[b0:b0 + L, :nh * HD]) is None, f"{what}: sequence {i} changes its out bits at place {j} of the pack"
        assert _first_diff(kc[i], kc2[j]) is None and _first_diff(vc[i], vc2[j]) is None, f"{what}: sequence {i} changes its cache bits at place {j} of the pack"
