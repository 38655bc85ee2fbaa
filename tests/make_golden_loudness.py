"""Writes tests/golden/loudness_kats.npz: for the seeded signals of tests/test_loudness_host.py, the K-weighted hop energies, the
400 ms block values and the BS.1770-4 integrated loudness, all in float64 through scipy.signal.lfilter — the yardstick the float32
restatement (and through it, bitwise, the device) is held to. scipy is needed here only, never by a test.

    python tests/make_golden_loudness.py
"""
import os
import sys

import numpy as np
from scipy.signal import lfilter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE); sys.path.insert(0, os.path.dirname(HERE))
from test_loudness_host import FS, HOP, SIGNALS, kweight_np, make_signal      # noqa: E402


def measure(x):
    sh, hp = kweight_np(FS)
    k = lfilter(hp[:3], hp[3:], lfilter(sh[:3], sh[3:], x.astype(np.float64)))
    hops = x.size // HOP
    e = (k[:hops * HOP] ** 2).reshape(hops, HOP).sum(axis=1)
    z = (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / (4.0 * HOP)
    ga = 10.0 ** ((-70.0 + 0.691) / 10.0)
    above = z[z > ga]
    gr = 0.1 * above.mean()
    kept = above[above > gr]
    return e, z, -0.691 + 10.0 * np.log10(kept.mean()), kept.size


def main():
    sh, hp = kweight_np(FS)
    out = {"names": np.array(list(SIGNALS)), "shelf_24k": sh, "highpass_24k": hp}
    for name, p in SIGNALS.items():
        x = make_signal(name)
        e, z, l, n = measure(x)
        out[name + "_seed"] = np.int64(p["seed"]); out[name + "_n"] = np.int64(x.size)
        out[name + "_e"] = e; out[name + "_z"] = z; out[name + "_lufs"] = np.float64(l); out[name + "_gated"] = np.int64(n)
        print(f"{name}: {x.size} samples, {z.size} blocks, {n} gated, {l:.6f} LUFS")
    path = os.path.join(HERE, "golden", "loudness_kats.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
