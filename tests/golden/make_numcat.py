#!/usr/bin/env python3
"""Record tests/golden/numcat.npz from the GENUINE reference's ParseFloat
(oracle/_ref/libdmlc_ref.so, as make_golden.gen_floats records floats.npz).

Run in the build container, after `make -C oracle ref`:
    python tests/golden/make_numcat.py

Data only: the float strings of the compact catalogue of tests/numcat.py
(every float class but frac_exhaustive, midpoint thinned to the 6 000 strings
closest to their midpoints; without the two unclosed "nan(" literals, on which the reference aborts) -> f32 bits and
bytes consumed.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.dirname(HERE)]
import numcat  # noqa: E402
from oracle import pyoracle as po  # noqa: E402


def main():
    strs = numcat.fixture_strings()
    assert not any("\0" in s for s in strs)
    bits, used = [], []
    for s in strs:
        v, n = po.ref_parse_float(s)
        bits.append(np.float32(v).view(np.uint32))
        used.append(n)
    path = os.path.join(HERE, "numcat.npz")
    np.savez_compressed(path, text=np.frombuffer("\0".join(strs).encode("latin-1"), dtype=np.uint8),
                        bits=np.array(bits, dtype=np.uint32), used=np.array(used, dtype=np.int32))
    print("numcat.npz:", len(strs), "strings,", os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
