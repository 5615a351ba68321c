"""CPU checks of the CSR -> dense conversion.

tests/emu/dense_check.cpp (ASan + UBSan, built by tests/emu/dense.mk) runs the
device tile body of dense_core.h with 256 host threads per tile, for every
index and value type, over column counts 1, 2, 3, 63, 64, 65 and C - 1, C,
C + 1, 2C + 3 (C cells per tile), 0 rows / 1 row / 1-3 row tiles with a partial
last one, both strides, a shifted output, duplicates, skewed rows, row
windows, dropped entries (also u64 indices >= 2^32), absent values and every
status flag, against a sequential loop in the program; whole buffers and the
status words must be equal.

The numpy model the GPU tests compare with (tests/dense_model.py) is pinned
here to three hand-written matrices."""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import dense_model as dmod

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "dense_check")


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_dense"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "dense.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_tile_body_equals_the_sequential_loop(report):
    m = re.search(r"cases (\d+), jobs (\d+), tiles (\d+), column-tiled (\d+), multi-row-tile (\d+), dropped (\d+), "
                  r"contiguous (\d+), strided (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    cases, jobs, tiles, coltiled, multirow, dropped, contiguous, strided, bad = map(int, m.groups())
    assert bad == 0, "\n".join(ln for ln in report.splitlines() if not ln.endswith("mismatches 0"))[-4000:]
    assert cases >= 150 and jobs >= 6 * 150 and tiles >= 1000, m.group(0)
    # each path was taken: column tiles, several row tiles, the dropped-entry atomics, both store forms
    assert coltiled > 0 and multirow > 0 and dropped > 0 and contiguous > 0 and strided > 0, m.group(0)


@pytest.mark.parametrize("types", ["u32/f32", "u32/i32", "u32/i64", "u64/f32", "u64/i32", "u64/i64"])
def test_every_type_pair_ran_every_case_group(report, types):
    lines = [ln for ln in report.splitlines() if ("/" + types + " ") in ln]
    groups = {ln.split("/")[0] for ln in lines}
    assert groups >= {"shape", "dense", "novalue", "dup", "skew", "window", "dropped", "flag"}, groups
    assert all(ln.endswith("mismatches 0") for ln in lines)
    flags = {int(re.search(r"flags (\d+)", ln).group(1)) for ln in lines if ln.startswith("flag/")}
    assert flags == {1, 2, 4}, flags
    if types.startswith("u64"):
        wide = [ln for ln in lines if ln.startswith("dropped/wide-index")]
        assert wide and int(re.search(r"dropped +(\d+)", wide[0]).group(1)) > 0


# ------------------------------------------------------------ the model --
def _run(offset, index, value, ncol, fill, dtype=np.float32, **kw):
    rows = len(offset) - 1
    buf = np.full(rows * ncol, 0xA5A5A5A5, dtype=np.uint32)
    fill_bits = int(np.array([fill], dtype=dtype).view(np.uint32)[0])
    out, status = dmod.to_dense(np.asarray(offset, np.uint64), np.asarray(index, np.uint32),
                                np.asarray(value, dtype), buf, value_dtype=dtype,
                                counts=(rows, len(index), len(value)), ncol=ncol, fill_bits=fill_bits, **kw)
    return out.view(dtype).reshape(rows, ncol), status


def test_model_label_column_csv_example():
    # "label,f0,f1\n1,2.5,3\n0,,4\n" with label_column=0 parses to offsets
    # [0,2,4,5], values [0,0,2.5,3,4]; an empty field pushes nothing but keeps its column, so the 4 has index 1
    d, status = _run([0, 2, 4, 5], [0, 1, 0, 1, 1], [0, 0, 2.5, 3, 4], 2, np.nan)
    want = np.array([[0, 0], [2.5, 3], [np.nan, 4]], dtype=np.float32)
    assert d.tobytes() == want.tobytes()
    assert status == [3, 0, dmod.NONE, 0]


def test_model_libsvm_without_values_gives_ones():
    # "1 0 3\n0 2\n": RowBlock::get_value returns 1 where there is no value array
    d, status = _run([0, 2, 3], [0, 3, 2], [], 4, 0.0)
    assert d.tobytes() == np.array([[1, 0, 0, 1], [0, 0, 1, 0]], dtype=np.float32).tobytes()
    assert status == [2, 0, dmod.NONE, 0]


def test_model_duplicate_index_last_wins_and_dropped_entries():
    # "1 3:1 3:2 3:5": cell 3 is 5
    d, status = _run([0, 3], [3, 3, 3], [1, 2, 5], 4, -1.0)
    assert d.tobytes() == np.array([[-1, -1, -1, 5]], dtype=np.float32).tobytes()
    assert status == [1, 0, dmod.NONE, 0]
    # the same row into 3 columns: all three entries are dropped, the first at position 0
    d, status = _run([0, 3], [3, 3, 3], [1, 2, 5], 3, -1.0)
    assert d.tobytes() == np.full((1, 3), -1, dtype=np.float32).tobytes()
    assert status == [1, 3, 0, 0]
