"""CPU check of the single-pass front half's classifier (fast_common.h
classify16_lut, quad_planes) by tests/emu/classify16_check.cpp (ASan + UBSan).

An interior tile classifies each 16-byte unit from its staging registers into
four 16-bit plane pieces, and the four lanes of a quad exchange them so that
lane j holds plane j's word of the 64-byte segment.  On more than 2M segments
-- every byte value alone and at every unit offset, then random mixes of the
grammar's alphabet with all 256 byte values -- the pieces, the words the
exchange's host form returns (planes D, N, C and the digit-plane words gw),
the ballot form of the tile's last segment and the post-halo's digit word must
equal classify64_lut / classify_dword_lut."""
import fcntl
import os
import re
import subprocess

import pytest

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "classify16_check")


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_classify16"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "classify16.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_pieces_and_exchange_equal_classify64(report):
    m = re.search(r"segments (\d+), with a byte >= 0x80 (\d+), with letters (\d+), "
                  r"with bytes outside the grammar (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    segs, hi, letters, outside, bad = map(int, m.groups())
    assert bad == 0, report[-4000:]
    assert segs >= 2 << 20, segs
    # the mixes reached every kind of segment, clean ones included
    assert hi > 1000 and letters > 1000 and 1000 < outside < segs - 1000, m.group(0)
