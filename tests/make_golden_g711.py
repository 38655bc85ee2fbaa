"""Writes tests/golden/g711_tables.npz: the ITU-T G.711 byte of every int16 value, as CPython's `audioop` compands it.

    ulaw[v + 32768] = audioop.lin2ulaw(<v as 2 little-endian bytes>, 2)      uint8[65536]
    alaw[v + 32768] = audioop.lin2alaw(<v as 2 little-endian bytes>, 2)      uint8[65536]

`audioop` is the yardstick that is independent of this project (the module left the standard library with Python 3.13: run
this with an interpreter that still has it). tests/test_g711.py reads the file and, where `audioop` imports, derives it again."""
import os
import sys

import numpy as np


def tables():
    import audioop
    v = np.arange(-32768, 32768, dtype=np.int64).astype("<i2").tobytes()
    ulaw = np.frombuffer(audioop.lin2ulaw(v, 2), dtype=np.uint8).copy()
    alaw = np.frombuffer(audioop.lin2alaw(v, 2), dtype=np.uint8).copy()
    assert ulaw.size == alaw.size == 65536
    return ulaw, alaw


def main():
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "g711_tables.npz")
    ulaw, alaw = tables()
    np.savez_compressed(out, ulaw=ulaw, alaw=alaw)
    print(f"wrote {out}: {os.path.getsize(out)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
