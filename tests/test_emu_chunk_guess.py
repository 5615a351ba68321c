"""CPU check of the single-pass tile prologue (fast_common.h): the one-trip
chunk list (chunk_guess_begin / chunk_guess_end) and the computed decoder
tables (init_dec_tables), by tests/emu/chunk_guess_check.cpp (ASan + UBSan).

For every tile it runs -- synthetic unit-start tables of 1, 2, 63, 64, 65, 257
and 5000 units: equal, cut back like InputSplit's, random with empty units,
one unit of 90 % of the text before / after tiny ones, one-line units filling
a tile with exactly kMaxCs and kMaxCs + 1 starts, starts at tlo - 1 / tlo /
thi - 1 / thi, a found unit in the window's last lanes -- the TileCommon fields
csl, cfloor, cnext, ncs, c_first, toomany and bad must equal a plain linear
scan of cs and, field for field, what the search form chunk_list() leaves.
The emulated init_dec_tables output must equal kDecTables byte for byte."""
import fcntl
import os
import re
import subprocess

import pytest

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "chunk_guess_check")


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_chunk_guess"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "chunk_guess.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_chunk_list_equals_linear_scan_and_search(report):
    m = re.search(r"tables (\d+), tiles (\d+), window (\d+), search (\d+), toomany (\d+), reloads (\d+), "
                  r"mismatches (\d+)", report)
    assert m, report[-2000:]
    tables, tiles, window, search, toomany, reloads, bad = map(int, m.groups())
    assert bad == 0, report[-4000:]
    # both ways were taken, and the rare ends of each were reached
    assert tables >= 40 and tiles >= 400 and window > 0 and search > 0 and toomany > 0 and reloads > 0, m.group(0)


@pytest.mark.parametrize("units", [1, 2, 63, 64, 65, 257, 5000])
def test_table_sizes_ran(report, units):
    rows = re.findall(r"^(\S+)\s+units\s+%d tiles\s+(\d+): window\s+(\d+) search\s+(\d+)" % units, report, re.M)
    assert {r[0].split("/")[0] for r in rows} >= {"equal", "cut", "random"}, rows
    for name, tiles, window, search in rows:
        assert int(tiles) == int(window) + int(search) and int(tiles) > 0, (name, tiles, window, search)
        if units >= 64 and name.split("/")[0] in ("equal", "cut"):
            assert int(search) == 0, (name, search)  # near-uniform units: the window brackets every tile


def test_guess_misses_fall_back(report):
    for name in ("big-first/65", "big-first/257", "big-first/5000", "big-last/5000", "last-lanes/60", "last-lanes/200"):
        m = re.search(r"^%s\s+units\s+\d+ tiles\s+\d+: window\s+\d+ search\s+(\d+)" % re.escape(name), report, re.M)
        assert m and int(m.group(1)) > 0, name
    for name in ("lines/0", "lines/300", "lines/small"):  # kMaxCs + 1 starts in a tile
        m = re.search(r"^%s\s.*toomany (\d+)" % re.escape(name), report, re.M)
        assert m and int(m.group(1)) > 0, name


def test_dec_tables_equal_constants(report):
    assert "dec tables: 328 bytes equal to kDecTables" in report and "dec tables differ" not in report
