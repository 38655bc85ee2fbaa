"""Inputs of the packed prefill attention tests (tests/test_gpu_prefill_pack_ops.py, -m gpu). TEST INFRASTRUCTURE — no test lives here.

A pack: sequences of unequal length, every one from position 0, laid end to end in one qkv matrix — what q3_attn_prefill_packed_ex
runs (the packed q/k-norm + RoPE + append, the packed plane split, one packed attention launch per kernel). Each sequence is also a
case of its own for q3_attn_prefill_ex (n_seq = 1, rps = its length, base_pos = 0) and for the float64 reference of
prefill_ops_cases.py (attn_reference): seq_case() gives that view of the same arrays."""
import functools

import numpy as np

import prefill_ops_cases as C
from prefill_ops_cases import GEN_T, X3, HD

MAX_SEQ = C.MAX_SEQ                      # four pages per row: page edges inside and pages behind every sequence that must keep their bits
RATIOS = [(2, 1), (2, 2)]                # the GQA ratios the GEMM prefill path admits (d_nh_ok)

# f32-MFMA kernel: query blocks of 64 / 128 rows, key tiles of 32 — one below, exact, one above, several blocks, and sequence starts
# (48, 112, 177, 306, 561) that are no multiple of 32, 64 or 128
LENS_T = (48, 64, 65, 129, 255, 50)
# bf16x3 kernel: query blocks of 128 / 256 rows
LENS_X3 = (256, 257, 385, 300)
# kernel = -1: each sequence by its length, two launches over one pack
LENS_MIXED = (60, 255, 256, 300, 129)

# (name, lengths, kernel argument, layout)
CASES = [
    ("t-paged", LENS_T, GEN_T, 1),
    ("x3-paged", LENS_X3, X3, 1),
    ("mixed-paged", LENS_MIXED, -1, 1),
    ("t-contiguous", LENS_T, GEN_T, 0),
    ("x3-contiguous", LENS_X3, X3, 0),
]


def kernel_of(kernel, length):
    """the kernel a sequence of the pack runs — and its solo launch must name"""
    return kernel if kernel >= 0 else (X3 if length >= 256 else GEN_T)


@functools.lru_cache(maxsize=None)
def pack_case(nh, nkv, lens):
    """read-only inputs of a pack: qkv [sum(lens)][(nh + 2 nkv) * 128], norm weights, the logical caches [n_seq][nkv][MAX_SEQ][128]
    (random everywhere: what lies at and behind a sequence's length must keep its bits)"""
    n = len(lens); rows = int(sum(lens))
    rng = np.random.default_rng(nh * 1000 + nkv * 100 + rows * 13 + n)
    qkv = rng.standard_normal((rows, (nh + 2 * nkv) * HD)).astype(np.float32)
    qw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kw = (1.0 + 0.1 * rng.standard_normal(HD)).astype(np.float32)
    kc = rng.standard_normal((n, nkv, MAX_SEQ, HD)).astype(np.float32)
    vc = rng.standard_normal((n, nkv, MAX_SEQ, HD)).astype(np.float32)
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    for a in (qkv, qw, kw, kc, vc, row0):
        a.setflags(write=False)
    return dict(nh=nh, nkv=nkv, lens=tuple(lens), row0=row0, qkv=qkv, qw=qw, kw=kw, kc=kc, vc=vc, max_seq=MAX_SEQ)


def seq_case(p, i):
    """sequence i of pack p as a case of prefill_ops_cases (attn_reference, q3_attn_prefill_ex): one sequence of rps = its length at base 0"""
    L = p["lens"][i]; r0 = int(p["row0"][i])
    return dict(nh=p["nh"], nkv=p["nkv"], rps=L, base=0, n_seq=1, max_seq=p["max_seq"], pos=np.arange(L, dtype=np.int64),
                qkv=p["qkv"][r0:r0 + L], qw=p["qw"], kw=p["kw"], kc=p["kc"][i:i + 1], vc=p["vc"][i:i + 1])


def pack_slots(p):
    """page slots [n_seq][4] over two slabs (prefill_page_slots: distinct, unordered, both slabs in every row)"""
    n = len(p["lens"])
    return C.prefill_page_slots(n, p["max_seq"] // C.PAGE, 2, p["nh"] * 1009 + p["nkv"] * 101 + int(sum(p["lens"])))


def permuted(p, order):
    """the same sequences in another pack order (views / copies of the same values)"""
    lens = tuple(p["lens"][i] for i in order)
    qkv = np.concatenate([p["qkv"][int(p["row0"][i]):int(p["row0"][i]) + p["lens"][i]] for i in order], 0)
    row0 = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
    return dict(nh=p["nh"], nkv=p["nkv"], lens=lens, row0=row0, qkv=qkv, qw=p["qw"], kw=p["kw"], kc=p["kc"][list(order)], vc=p["vc"][list(order)],
                max_seq=p["max_seq"])
