"""Op-level tests of prefill attention over PAGED K/V (-m gpu): the form prefill_gemm runs by default. q3_attn_prefill_ex with
layout = 1 scatters the logical cache of one layer over two pattern-filled slabs of KvPool's geometry (the page table between
them, entries beyond a row's pages naming its first page), then runs the launches of the contiguous tests — k_qknorm_rope_kv
appending through kv_krow into rotated rows of scattered pages, k_kv_planes into a NaN-filled buffer, ONE launch_attn_prefill
(k_attn_prefill, k_attn_prefill_mfma, k_attn_prefill_t, k_attn_prefill_x3 reading every key through kv_krow / kv_vd), the two-halves
merge — and gathers the cache back. Cases, the slot helper and the float64 reference live in prefill_ops_cases.py (paged_cases():
each row names the rule it is chosen against); the D_REF recomputation, the helper's properties, every refusal of the entry and the
proof that the bound sees a key dropped, duplicated or taken from the neighbour's page are in test_prefill_ops_reference.py.

Checked per launch (the message names the case, kernel and halves, the layer and the first differing element / stray offset):
  * `out` and the appended K rows against float64 within 4 * D_REF / 4 * D_REF_K (softmax stress: 4 * D_REF_STRESS) — the constants
    of the contiguous tests; numpy float32 over these cases stays below them (recomputed on the CPU);
  * the appended V rows are the v part of qkv bit for bit, every other logical cache element keeps its bits (shared pages included);
  * stray == 0: nothing in either slab outside the cache rows of the layer changed — other layers, unused slots, run padding;
  * `out` and both caches are bit-identical to layout = 0 with the same kernel and halves on the same inputs; the shared-prefix
    case (sequences 0 and 1 name the same physical pages 0 and 1) also to the same case with private copies of those pages;
  * the rotations used lie in 0..127 and differ between the pages of a row.

Measured on an MI355X (the module prints these as it ends), worst deviation in units of D_REF / D_REF_K, each held to a bound of 4:
  k_attn_prefill (VALU) 0.44, k_attn_prefill_mfma 1.50, k_attn_prefill_t 1.52, k_attn_prefill_x3 1.21; appended K rows 0.80 — the
  figures of the contiguous tests, as bit-identity demands;
  the 8192-position case: k_attn_prefill_t over two halves 1.45, k_attn_prefill_x3 over one half 1.73 (2.79e-6 of the case's
  maximum), over two halves 1.12; appended K rows 0.57.
Every case passed as first run: no kernel change came out of this file."""
import os

import numpy as np
import pytest

import qwen3_tts_rs_amd as q
import prefill_ops_cases as C
from prefill_ops_cases import VALU, GEN2, GEN_T, X3, HD, EPS, SENT, D_REF_K

pytestmark = pytest.mark.gpu

# the cases are chosen against the DEFAULT dispatch and the paged cache: these knobs would silently move them elsewhere
assert [k for k in os.environ if k.startswith("Q3_PREFILL_ATTN_") or k.startswith("Q3_GEMM_") or k == "Q3_KV_CONTIGUOUS"] == [], \
    "prefill / KV layout knobs set: the cases would not reach the kernels and the layout they name"

KERNEL_NAMES = {VALU: "k_attn_prefill", GEN2: "k_attn_prefill_mfma", GEN_T: "k_attn_prefill_t", X3: "k_attn_prefill_x3"}
WORST = {}          # (kernel, "long" | "") -> [out dev / D_REF, K row dev / D_REF_K]

BY_KEY = {}
for (_key, _kernel, _halves, _n_layers, _layer) in C.paged_cases():
    BY_KEY.setdefault(_key, []).append((_kernel, _halves, _n_layers, _layer))


def _kid(key):
    nh, nkv, rps, base, n_seq, stress, max_seq, shared = key
    return f"nh{nh}-nkv{nkv}-rps{rps}-base{base}-seq{n_seq}" + ("-stress" if stress else "") + (f"-shared{shared}" if shared else "") + \
        (f"-max{max_seq}" if max_seq != C.MAX_SEQ else "")


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for (kernel, tag) in sorted(WORST):
        d, dk = WORST[(kernel, tag)]
        print(f"\nworst deviation over pages, {KERNEL_NAMES[kernel]}{' (8192 positions)' if tag else ''}: out {d:.2f} D_REF (bound 4), "
              f"appended K rows {dk:.2f} D_REF_K (bound 4)", end="")
    print()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _first_diff(a, b):
    d = np.argwhere(_bits(a) != _bits(b))
    return None if len(d) == 0 else tuple(int(i) for i in d[0])


def _launch(key, kernel, halves, layout, n_layers=1, layer=0, private=False):
    c = C.attn_case(*key)
    nh, nkv, n_seq = c["nh"], c["nkv"], c["n_seq"]
    rc, rs = C.rope(c["max_seq"])
    out_in = np.full((n_seq * c["rps"], nh * HD + 4), SENT, dtype=np.float32)
    kw = dict(kernel=kernel, halves=halves, out=out_in)
    if layout:
        kw.update(layout=1, n_layers=n_layers, layer=layer, n_slabs=2, page_slots=C.case_page_slots(key, private))
    return q.attn_prefill_ex(c["qkv"], n_seq, c["base"], c["qw"], c["kw"], EPS, rc, rs, c["kc"], c["vc"], nh, nkv, **kw)


def _check(key, kernel, halves, n_layers, layer):
    c = C.attn_case(*key)
    o64, k64 = C.attn_ref64(key)
    nh, nkv, rps, base, n_seq = c["nh"], c["nkv"], c["rps"], c["base"], c["n_seq"]
    rows = n_seq * rps
    d_ref = C.case_d_ref(key)
    what = f"{_kid(key)} {KERNEL_NAMES[kernel]} halves={halves} layer {layer} of {n_layers}"
    out, kc, vc, path, info = _launch(key, kernel, halves, 1, n_layers, layer)
    assert path == (kernel, halves), f"{what}: ran {path}"
    # stray writes first: they name the fault most directly
    assert info["stray"] == 0, f"{what}: {info['stray']} slab elements outside the cache rows of the layer changed, the first at offset {info['stray_at']}"
    assert (_bits(out[:, nh * HD:]) == _bits(np.full((rows, 4), SENT))).all(), f"{what}: out written beyond nh * 128 columns"
    out = out[:, :nh * HD]
    bad = np.argwhere(~np.isfinite(out))
    assert len(bad) == 0, f"{what}: {len(bad)} non-finite outputs, the first at {tuple(bad[0])} (an invisible row read in: NaN planes or records)"
    dev = float(np.abs(out - o64).max() / np.abs(o64).max())
    k_new = kc[:, :, base:base + rps].transpose(0, 2, 1, 3).reshape(rows, nkv, HD)
    v_new = vc[:, :, base:base + rps].transpose(0, 2, 1, 3).reshape(rows, nkv, HD)
    dev_k = float(np.abs(k_new - k64).max() / np.abs(k64).max())
    w = WORST.setdefault((kernel, "long" if C.is_long(key) else ""), [0.0, 0.0])
    w[0] = max(w[0], dev / d_ref); w[1] = max(w[1], dev_k / D_REF_K)
    print(f"{what}: out dev {dev:.3e} = {dev / d_ref:.2f} D_REF (bound 4), K row dev {dev_k:.3e} = {dev_k / D_REF_K:.2f} D_REF_K (bound 4)")
    at = np.unravel_index(np.abs(out - o64).argmax(), out.shape)
    assert dev <= 4 * d_ref, f"{what}: out deviates {dev:.3e} > {4 * d_ref:.3e}, worst at {tuple(int(i) for i in at)}"
    at = np.unravel_index(np.abs(k_new - k64).argmax(), k_new.shape)
    assert dev_k <= 4 * D_REF_K, f"{what}: appended K rows deviate {dev_k:.3e} > {4 * D_REF_K:.3e}, worst at {tuple(int(i) for i in at)}"
    # cache contents
    v_in = c["qkv"][:, (nh + nkv) * HD:].reshape(rows, nkv, HD)
    assert _first_diff(v_new, v_in) is None, f"{what}: appended V rows are not the v part of qkv, first at (row, kv head, d) {_first_diff(v_new, v_in)}"
    for name, got, want in (("K", kc, c["kc"]), ("V", vc, c["vc"])):
        g = got.copy(); g[:, :, base:base + rps] = want[:, :, base:base + rps]
        assert _first_diff(g, want) is None, f"{what}: {name} cache changed outside the appended rows, first at (seq, kv head, pos, d) {_first_diff(g, want)}"
    # rotation
    rot = info["rot_used"]
    assert ((rot >= 0) & (rot < 128)).all(), f"{what}: rotation outside 0..127"
    assert all(len(set(rot[s, :, g].tolist())) > 1 for s in range(n_seq) for g in range(nkv)), f"{what}: one rotation for every page of a row"
    # bit-identity with the contiguous layout
    out0, kc0, vc0, path0 = _launch(key, kernel, halves, 0)
    assert path0 == path
    for name, a, b in (("out", out, out0[:, :nh * HD]), ("K cache", kc, kc0), ("V cache", vc, vc0)):
        assert _first_diff(a, b) is None, f"{what}: {name} differs from the contiguous layout, first at {_first_diff(a, b)}"
    if key[7]:          # shared prefix pages against private copies of them
        slots = C.case_page_slots(key)
        assert (slots[0, :key[7]] == slots[1, :key[7]]).all()
        out1, kc1, vc1, _, info1 = _launch(key, kernel, halves, 1, n_layers, layer, private=True)
        assert info1["stray"] == 0, f"{what} (private pages): stray writes, the first at offset {info1['stray_at']}"
        for name, a, b in (("out", out, out1[:, :nh * HD]), ("K cache", kc, kc1), ("V cache", vc, vc1)):
            assert _first_diff(a, b) is None, f"{what}: {name} differs between shared and private prefix pages, first at {_first_diff(a, b)}"


@pytest.mark.parametrize("key", list(BY_KEY), ids=_kid)
def test_paged_prefill_attention(key):
    for (kernel, halves, n_layers, layer) in BY_KEY[key]:
        _check(key, kernel, halves, n_layers, layer)

