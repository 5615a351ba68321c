"""CPU checks of the CSR -> bin codes conversion.

tests/emu/bins_check.cpp (ASan + UBSan, built by tests/emu/bins.mk) runs the
device tile body of bins_core.h with 256 host threads per tile, for both index
types and the three code widths, over column counts 1, 2, 3, 15, 16, 17, 63,
64, 65 and C - 1, C, C + 1, 2C + 3 (C cells per tile), 0 rows / 1 row / 1-3
row tiles with a partial last one, both strides, an output shifted by 1, 3 and
15 elements, cut counts 0, 1, 2, 3, 255, 256, 257, values on and next to the
cuts, +-0, +-inf, a denormal and NaN, duplicates, row windows, dropped
entries, absent values, global ids and every status flag, against a
sequential loop in the program; whole buffers and the eight status words must
be equal, and the cut array ends at n_cuts so a read past it is a heap
overflow.

The numpy model the GPU tests compare with (tests/bins_model.py) is pinned
here to hand-written matrices."""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import bins_model as bmod

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "bins_check")
NAN = float("nan")


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_bins"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "bins.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_tile_body_equals_the_sequential_loop(report):
    m = re.search(r"cases (\d+), jobs (\d+), tiles (\d+), column-tiled (\d+), multi-row-tile (\d+), dropped (\d+), "
                  r"contiguous (\d+), strided (\d+), lds-cuts (\d+), lds-groups (\d+), global-cuts (\d+), "
                  r"row-too-long (\d+), code-range (\d+), "
                  r"cut-ptr (\d+), nan (\d+), unbinned (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    (cases, jobs, tiles, coltiled, multirow, dropped, contiguous, strided, lds, lds_groups, glob, too_long,
     code_range, cut_ptr, nan, unbinned, bad) = map(int, m.groups())
    assert bad == 0, "\n".join(ln for ln in report.splitlines() if not ln.endswith("mismatches 0"))[-4000:]
    assert cases >= 200 and jobs >= 6 * 200 and tiles >= 1000, m.group(0)
    # each path was taken: column tiles, several row tiles, the dropped-entry atomics, both store forms, cuts
    # staged in LDS (in one column group and in several) and cuts read from global memory, a tile refused for a
    # row too long, both new flags and both new counters
    assert min(coltiled, multirow, dropped, contiguous, strided, lds, lds_groups, glob, too_long, code_range, cut_ptr,
               nan, unbinned) > 0, \
        m.group(0)


@pytest.mark.parametrize("types", ["u32/c1", "u32/c2", "u32/c4", "u64/c1", "u64/c2", "u64/c4"])
def test_every_type_pair_ran_every_case_group(report, types):
    lines = [ln for ln in report.splitlines() if ("/" + types + " ") in ln]
    groups = {ln.split("/")[0] for ln in lines}
    assert groups >= {"shape", "dense", "novalue", "dup", "skew", "window", "dropped", "flag", "toolong", "range",
                      "cutptr", "scattered", "global"}, groups
    assert all(ln.endswith("mismatches 0") for ln in lines)
    flag = lambda ln: int(re.search(r"flags (\d+)", ln).group(1))  # noqa: E731
    # (the dense bits; the offset-cap case's 257-cut columns also overflow a byte: bit 4 is checked below)
    assert {flag(ln) & 15 for ln in lines if ln.startswith("flag/")} == {1, 2, 4}
    assert all(flag(ln) & 32 for ln in lines if ln.startswith("cutptr/"))
    # ROW_TOO_LONG: the flag, every row of the window counted, with and without column tiling
    long_rows = [ln for ln in lines if ln.startswith("toolong/")]
    assert len(long_rows) == 2 and all(flag(ln) & 15 == 8 for ln in long_rows), long_rows
    assert {int(re.search(r"coltiles (\d+)", ln).group(1)) > 1 for ln in long_rows} == {False, True}
    # 257 cuts overflow one byte only; 256 cuts meet missing_code 255 in one byte only; 255 cuts never
    want = {"range/257cuts": types.endswith("c1"), "range/256cuts": types.endswith("c1"), "range/255cuts": False,
            "range/missing=1": True}
    for name, flagged in want.items():
        ln = [x for x in lines if x.startswith(name + "/")]
        assert len(ln) == 1 and bool(flag(ln[0]) & 16) == flagged, ln
    if types.startswith("u64"):
        wide = [ln for ln in lines if ln.startswith("dropped/wide-index")]
        assert wide and int(re.search(r"dropped +(\d+)", wide[0]).group(1)) > 0


# ------------------------------------------------------------ the model --
def _binding_agrees():
    """The model speaks of the call the library exports: the same flag bits, status words and widths."""
    import dmlc_amd
    assert "dmlc_amd_to_bins" in dmlc_amd.EXPORTED_SYMBOLS
    assert (dmlc_amd.BINS_FLAG_CODE_RANGE, dmlc_amd.BINS_FLAG_CUT_PTR) == (bmod.FLAG_CODE_RANGE, bmod.FLAG_CUT_PTR)
    assert (dmlc_amd.BINS_ROWS, dmlc_amd.BINS_DROPPED, dmlc_amd.BINS_FIRST, dmlc_amd.BINS_FLAGS, dmlc_amd.BINS_NAN,
            dmlc_amd.BINS_UNBINNED) == (bmod.ROWS, bmod.DROPPED, bmod.FIRST, bmod.FLAGS, bmod.NAN, bmod.UNBINNED)
    assert dmlc_amd.bins_geometry() == dmlc_amd.dense_geometry()  # the window and the tiles are to_dense's


def _run(offset, index, value, cut_ptr, cut_value, ncol, dtype=np.uint8, **kw):
    _binding_agrees()
    rows = len(offset) - 1
    buf = np.full(rows * ncol, 0xA5, dtype=dtype)
    out, status = bmod.to_bins(np.asarray(offset, np.uint64), np.asarray(index, np.uint32),
                               np.asarray(value, np.float32), buf, np.asarray(cut_ptr, np.uint32),
                               np.asarray(cut_value, np.float32), counts=(rows, len(index), len(value)), ncol=ncol,
                               **kw)
    return out.reshape(rows, ncol).tolist(), status


def test_model_label_column_csv_example():
    # "label,f0,f1\n1,2.5,3\n0,,4\n" with label_column=0 parses to offsets [0,2,4,5], values
    # [0,0,2.5,3,4] (the header row reads as zeros); the 4 of the last row has index 1.
    # column 0 cuts [1, 2.5, 3]: 0 -> 0, 2.5 -> 2 (a value on a cut belongs to the bin above it);
    # column 1 cuts [3.5, 5]: 0 -> 0, 3 -> 0, 4 -> 1
    codes, status = _run([0, 2, 4, 5], [0, 1, 0, 1, 1], [0, 0, 2.5, 3, 4], [0, 3, 5], [1, 2.5, 3, 3.5, 5], 2)
    assert codes == [[0, 0], [2, 0], [255, 1]]
    assert status == [3, 0, bmod.NONE, 0, 0, 0, 0, 0]
    # the same with global ids in two bytes: column 1's codes start at cut_ptr[1] = 3
    codes, status = _run([0, 2, 4, 5], [0, 1, 0, 1, 1], [0, 0, 2.5, 3, 4], [0, 3, 5], [1, 2.5, 3, 3.5, 5], 2,
                         dtype=np.uint16, global_ids=True)
    assert codes == [[0, 3], [2, 3], [65535, 4]]


def test_model_libsvm_duplicate_cell_whose_last_entry_is_nan():
    # "1 3:1 3:2 3:nan 0:7\n0 3:9 3:0.5": row 0's cell 3 is the NaN (the last entry wins) and counts as NaN, not
    # as 2; cell 0 holds 7, above every cut: the last bin, 2 - 1.  Row 1's cell 3 is 0.5 -> below the first cut
    codes, status = _run([0, 4, 6], [3, 3, 3, 0, 3, 3], [1, 2, NAN, 7, 9, 0.5], [0, 2, 2, 2, 5],
                         [1, 5, 1, 2, 8], 4)
    assert codes == [[1, 255, 255, 255], [255, 255, 255, 0]]
    assert status == [2, 0, bmod.NONE, 0, 1, 0, 0, 0]
    # an entry at column 4 is dropped, as in the dense model
    codes, status = _run([0, 2], [4, 3], [1, 2], [0, 2, 2, 2, 5], [1, 5, 1, 2, 8], 4)
    assert codes == [[255, 255, 255, 2]] and status == [1, 1, 0, 0, 0, 0, 0, 0]


def test_model_column_without_cuts_and_bad_cut_ptr():
    # column 1 owns no cuts: its cells are missing and counted as unbinned -- the NaN in it too (not as NaN)
    codes, status = _run([0, 3, 5], [0, 1, 2, 1, 2], [0.0, 4.0, -np.inf, NAN, np.inf], [0, 1, 1, 3], [0, -1, 1], 3,
                         missing=9)
    assert codes == [[0, 9, 0], [9, 9, 1]]  # -0/0 on the cut 0 -> min(1, 0) = 0; -inf -> 0; +inf -> m - 1 = 1
    assert status == [2, 0, bmod.NONE, 0, 0, 2, 0, 0]
    # cut_ptr descending at column 1 / past n_cuts at column 2: unbinned and the CUT_PTR flag
    codes, status = _run([0, 3], [0, 1, 2], [5, 5, 5], [0, 2, 1, 3], [1, 2, 3], 3)
    assert codes == [[1, 255, 1]] and status == [1, 0, bmod.NONE, 32, 0, 1, 0, 0]
    codes, status = _run([0, 3], [0, 1, 2], [5, 5, 5], [0, 1, 2, 4], [1, 2, 3], 3)
    assert codes == [[0, 0, 255]] and status == [1, 0, bmod.NONE, 32, 0, 1, 0, 0]
    # a column whose cut_ptr is bad but which holds no entry sets nothing
    codes, status = _run([0, 1], [0], [5], [0, 1, 2, 4], [1, 2, 3], 3)
    assert codes == [[0, 255, 255]] and status == [1, 0, bmod.NONE, 0, 0, 0, 0, 0]


def test_model_code_range_and_no_values():
    # no value array: every present cell is 1.0f; cuts [0, 1, 2] -> upper bound 2
    codes, status = _run([0, 2, 3], [0, 3, 2], [], [0, 3, 3, 6, 9], [0, 1, 2, 0, 1, 2, 5, 6, 7], 4)
    assert codes == [[2, 255, 255, 0], [255, 255, 2, 255]]
    assert status == [2, 0, bmod.NONE, 0, 0, 0, 0, 0]
    # a code equal to missing_code is stored as missing_code and flagged
    codes, status = _run([0, 2, 3], [0, 3, 2], [], [0, 3, 3, 6, 9], [0, 1, 2, 0, 1, 2, 5, 6, 7], 4, missing=2)
    assert codes == [[2, 2, 2, 0], [2, 2, 2, 2]] and status[3] == 16
    # 257 cuts: the top code 256 does not fit a byte, fits two
    cuts = np.arange(257, dtype=np.float32)
    codes, status = _run([0, 2], [0, 1], [255.5, 256.0], [0, 257, 514], np.concatenate([cuts, cuts]), 2)
    assert codes == [[255, 255]] and status[3] == 16
    codes, status = _run([0, 2], [0, 1], [255.5, 256.0], [0, 257, 514], np.concatenate([cuts, cuts]), 2,
                         dtype=np.uint16)
    assert codes == [[256, 256]] and status[3] == 0
