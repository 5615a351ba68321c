"""CPU checks of the CSC transpose (dmlc_amd_to_csc).

tests/emu/csc_check.cpp (ASan + UBSan, built by tests/emu/csc.mk) runs the
device tile bodies of csc_core.h -- hist, scan, scatter, bounds -- with 256 host
threads per tile over entry counts in {0, 1, T-1, T, T+1, 2T+1} (T entries per
tile), 257T+3 entries (the scan's per-thread run of 2 tiles), every pass count
(ncol from 1 to 2^24 + 1), the stability cases, dropped entries (also 2^32 + c
with 64-bit indices), empty rows (10000 of them inside one tile: the offsets
that do not fit LDS), one row of 3T+5 entries, row windows, absent arrays, a
capacity one short and every status flag, against a sequential loop in the
program; whole buffers, guard words and the status words must be equal.

The numpy model the GPU tests compare with (tests/csc_model.py) is pinned here
to three hand-written matrices."""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import csc_model as cm

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "csc_check")


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_csc"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "csc.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_tile_bodies_equal_the_sequential_loop(report):
    m = re.search(r"cases (\d+), jobs (\d+), tiles (\d+), multi-tile (\d+), long-scan (\d+), multi-pass (\d+), "
                  r"dropped (\d+), overflow (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    cases, jobs, tiles, multitile, longscan, multipass, dropped, overflow, bad = map(int, m.groups())
    assert bad == 0, "\n".join(ln for ln in report.splitlines() if not ln.endswith("mismatches 0"))[-4000:]
    assert cases >= 40 and jobs >= 100 and tiles >= 400, m.group(0)
    # each path was taken: several tiles, a scan run longer than one tile, several passes, drops, an overflow
    assert multitile > 0 and longscan > 0 and multipass > 0 and dropped > 0 and overflow > 0, m.group(0)


def test_every_pass_count_ran(report):
    want = {1: 1, 2: 1, 255: 1, 256: 1, 257: 2, 65536: 2, 65537: 3, 1 << 24: 3, (1 << 24) + 1: 4}
    for ncol, p in want.items():
        lines = [ln for ln in report.splitlines() if ln.startswith("ncol/%d/" % ncol)]
        assert lines and all(int(re.search(r"passes (\d)", ln).group(1)) == p for ln in lines), (ncol, lines)
        assert cm.passes(ncol) == p


@pytest.mark.parametrize("widths", ["u32/v4", "u64/v4", "u32/v8", "u64/v8"])
def test_every_width_combination_ran_the_small_case_groups(report, widths):
    lines = [ln for ln in report.splitlines() if ("/" + widths + " ") in ln]
    groups = {ln.split("/")[0] for ln in lines}
    want = {"count", "drop", "absent", "cap", "flag"}
    if widths in ("u32/v4", "u64/v8"):
        want |= {"ncol", "stable", "rows", "window"}
    if widths == "u32/v4":
        want.add("scanrun")
    assert groups >= want, groups
    assert all(ln.endswith("mismatches 0") for ln in lines)
    flags = {int(re.search(r"flags +(\d+)", ln).group(1)) for ln in lines if ln.startswith("flag/")}
    assert flags >= {1, 2, 4}, flags
    caps = [ln for ln in lines if ln.startswith("cap/")]
    assert len(caps) >= 2 and all(int(re.search(r"flags +(\d+)", ln).group(1)) & 8 for ln in caps)
    if widths.startswith("u64"):
        assert any(ln.startswith("drop/2^32+c") for ln in lines)


# ------------------------------------------------------------ the model --
U32, U64 = np.uint32, np.uint64
SENT = 0xA5A5A5A5
SENT64 = 0xA5A5A5A5A5A5A5A5


def _bufs(ncol, cap, value=True, pos=True, extra=2):
    """Sentinel-filled outputs with `extra` words past each capacity."""
    return {"col_offset": np.full(ncol + 1 + extra, SENT64, U64), "row": np.full(cap + extra, SENT, U32),
            "value": np.full(cap + extra, SENT, U32) if value else None,
            "pos": np.full(cap + extra, SENT64, U64) if pos else None, "cap": cap}


def _f32(*v):
    return np.array(v, dtype=np.float32).view(U32)


def test_model_csv_with_a_label_column():
    # "label,f0,f1\n1,2.5,3\n0,,4\n" with label_column=0 parses to offsets [0,2,4,5],
    # indices [0,1,0,1,1], values [0,0,2.5,3,4] (the header row's text is 0)
    off, idx, val = np.array([0, 2, 4, 5], U64), np.array([0, 1, 0, 1, 1], U32), _f32(0, 0, 2.5, 3, 4)
    out, status = cm.to_csc(off, idx, val, _bufs(2, 5), counts=(3, 5, 5), ncol=2)
    assert list(out["col_offset"]) == [0, 2, 5, SENT64, SENT64]
    assert list(out["row"]) == [0, 1, 0, 1, 2, SENT, SENT]
    assert out["value"].tolist() == _f32(0, 2.5, 0, 3, 4).tolist() + [SENT, SENT]
    assert list(out["pos"]) == [0, 2, 1, 3, 4, SENT64, SENT64]
    assert status == [5, 0, cm.NONE, 0]
    # rows 1 .. 2 only: row ids are relative to the window, positions stay absolute
    out, status = cm.to_csc(off, idx, val, _bufs(2, 3), counts=(3, 5, 5), ncol=2, row_begin=1)
    assert list(out["col_offset"][:3]) == [0, 1, 3] and list(out["row"][:3]) == [0, 0, 1]
    assert list(out["pos"][:3]) == [2, 3, 4] and status == [3, 0, cm.NONE, 0]
    # one column: f1 is dropped, the first dropped position is 1
    out, status = cm.to_csc(off, idx, val, _bufs(1, 5), counts=(3, 5, 5), ncol=1)
    assert list(out["col_offset"][:2]) == [0, 2] and list(out["row"]) == [0, 1] + [SENT] * 5
    assert status == [2, 3, 1, 0]
    # an empty window, and a failed parse: col_offset all 0, nothing else written
    for kw in (dict(max_rows=0), dict(row_begin=3), dict(error=3)):
        out, status = cm.to_csc(off, idx, val, _bufs(2, 5), counts=(3, 5, 5), ncol=2, **kw)
        assert list(out["col_offset"]) == [0, 0, 0, SENT64, SENT64] and (out["row"] == SENT).all()
        assert status == [0, 0, cm.NONE, cm.FLAG_ERROR if "error" in kw else 0]


def test_model_libsvm_with_a_duplicate_cell_and_no_values():
    # "1 0 3\n0 2\n1 3 3 1\n": row 2 names column 3 twice; no value array
    off, idx = np.array([0, 2, 3, 6], U64), np.array([0, 3, 2, 3, 3, 1], U32)
    out, status = cm.to_csc(off, idx, None, _bufs(4, 6), counts=(3, 6, 0), ncol=4)
    assert list(out["col_offset"][:5]) == [0, 1, 2, 3, 6]
    assert list(out["row"][:6]) == [0, 2, 1, 0, 2, 2]
    assert list(out["pos"][:6]) == [0, 5, 2, 1, 3, 4]  # the duplicates in file order
    assert (out["value"] == SENT).all()  # neither read nor written
    assert status == [6, 0, cm.NONE, 0]
    # one entry short: col_offset and the status stay exact, nothing at or past the capacity is written
    out, status = cm.to_csc(off, idx, None, _bufs(4, 5), counts=(3, 6, 0), ncol=4)
    assert list(out["col_offset"][:5]) == [0, 1, 2, 3, 6] and list(out["row"]) == [0, 2, 1, 0, 2, SENT, SENT]
    assert status == [6, 0, cm.NONE, cm.FLAG_CAPACITY]


def test_model_libfm_pos_moves_the_fields():
    # "1 0:1:0.5 2:3:1.5\n0 1:2:2.5\n": fields [0,2,1], indices [1,3,2]
    off, fld, idx, val = np.array([0, 2, 3], U64), np.array([0, 2, 1], U32), np.array([1, 3, 2], U32), _f32(.5, 1.5, 2.5)
    out, status = cm.to_csc(off, idx, val, _bufs(4, 3), counts=(2, 3, 3), ncol=4)
    assert list(out["col_offset"][:5]) == [0, 0, 1, 2, 3] and list(out["row"][:3]) == [0, 1, 0]
    assert out["value"][:3].tolist() == _f32(.5, 2.5, 1.5).tolist()
    pos = out["pos"][:3].astype(np.int64)
    assert list(pos) == [0, 2, 1] and list(fld[pos]) == [0, 1, 2]
    assert status == [3, 0, cm.NONE, 0]
    # ncol = 3: index 3 (position 1) is dropped
    out, status = cm.to_csc(off, idx, val, _bufs(3, 3), counts=(2, 3, 3), ncol=3)
    assert list(out["col_offset"][:4]) == [0, 0, 1, 2] and list(out["pos"]) == [0, 2, SENT64, SENT64, SENT64]
    assert status == [2, 1, 1, 0]
    # a value count that fits no RowBlock
    out, status = cm.to_csc(off, idx, val, _bufs(4, 3), counts=(2, 3, 2), ncol=4)
    assert list(out["col_offset"][:5]) == [0] * 5 and status == [0, 0, cm.NONE, cm.FLAG_VALUE_COUNT]
