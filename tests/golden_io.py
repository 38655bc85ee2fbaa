"""Fixture archives under tests/golden/ stay below 1 MiB per file. An archive whose arrays would make it larger is written
as <stem>.npz plus <stem>.part1.npz, <stem>.part2.npz, ...; an array too large for one piece is cut along its first axis
into <key>.chunk0, <key>.chunk1, ... `load` returns the arrays of all pieces, chunked ones joined again, exactly as saved."""
import glob
import os
import re

import numpy as np

FILE_LIMIT = 1 << 20
_PIECE_BYTES = FILE_LIMIT - (64 << 10)       # raw bytes per piece: deflate never grows them past the zip overhead


def save(path, **arrays):
    """np.savez_compressed(path, **arrays), split into pieces of at most FILE_LIMIT bytes each."""
    items = []
    for key, a in arrays.items():
        a = np.asarray(a)
        if a.nbytes <= _PIECE_BYTES // 2 or a.ndim == 0:
            items.append((key, a))
            continue
        rows = max(1, (_PIECE_BYTES // 2) // max(1, a.nbytes // a.shape[0]))
        for i, r0 in enumerate(range(0, a.shape[0], rows)):
            items.append((f"{key}.chunk{i}", a[r0:r0 + rows]))
    pieces, cur, size = [], {}, 0
    for key, a in items:
        if cur and size + a.nbytes > _PIECE_BYTES:
            pieces.append(cur); cur, size = {}, 0
        cur[key] = a; size += a.nbytes
    pieces.append(cur)
    stem = path[:-4] if path.endswith(".npz") else path
    for old in glob.glob(glob.escape(stem) + ".part*.npz"):
        os.remove(old)
    for i, piece in enumerate(pieces):
        out = stem + (".npz" if i == 0 else f".part{i}.npz")
        np.savez_compressed(out, **piece)
        assert os.path.getsize(out) <= FILE_LIMIT, (out, os.path.getsize(out))


def load(path):
    """The arrays of `path` and its .partN pieces, as a dict."""
    stem = path[:-4] if path.endswith(".npz") else path
    parts = sorted(glob.glob(glob.escape(stem) + ".part*.npz"), key=lambda p: int(re.search(r"\.part(\d+)\.npz$", p).group(1)))
    out, chunks = {}, {}
    for p in [stem + ".npz"] + parts:
        with np.load(p) as z:
            for key in z.files:
                m = re.fullmatch(r"(.+)\.chunk(\d+)", key)
                if m:
                    chunks.setdefault(m.group(1), []).append((int(m.group(2)), z[key]))
                else:
                    out[key] = z[key]
    for key, cs in chunks.items():
        out[key] = np.concatenate([a for _, a in sorted(cs, key=lambda c: c[0])], axis=0)
    return out
