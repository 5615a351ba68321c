"""CPU checks of the quantile cuts (dmlc_amd_make_cuts).

tests/emu/cuts_check.cpp (ASan + UBSan, built by tests/emu/cuts.mk) runs the
device tile bodies of cuts_core.h -- hist, scan, scatter per digit pass, then
bounds, count, ptr, write -- with 256 host threads per tile over entry counts in
{0, 1, T-1, T, T+1, 2T+1} (T entries per tile), 257T+3 entries (the scan's
per-thread run of 2 tiles), ncol from 1 to 65537 (one to three column passes)
with empty columns first, last and in the middle, max_bin in {1, 2, 3, 255, 256,
257, 4096}, columns of 1, 2, B-1, B, B+1 samples, an all-equal column, a column
of 3T+5 samples among columns of one, keys that differ in one byte only (each of
the four), keys that tie across columns, the float edges (signed zeros,
infinities, FLT_MAX, denormals, NaNs of both signs), dropped entries (also 2^32
+ c with 64-bit indices), absent values, row windows, a capacity one short of
and equal to N_CUTS, max_entries one short of the window and every flag bit,
against a sequential loop in the program; cut_ptr with its guard words,
cut_value at exactly its capacity and the eight status words must be equal.

The numpy model the GPU tests compare with (tests/cuts_model.py) is pinned here
to hand-written columns."""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import bins_model as bm
import cuts_model as qm

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "cuts_check")
U32, U64 = np.uint32, np.uint64
SENT = 0xA5A5A5A5


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_cuts"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "cuts.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_tile_bodies_equal_the_sequential_loop(report):
    m = re.search(r"cases (\d+), jobs (\d+), tiles (\d+), multi-tile (\d+), long-scan (\d+), multi-pass (\d+), "
                  r"dropped (\d+), nan (\d+), dedupe (\d+), overflow (\d+), big-bin (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    cases, jobs, tiles, multitile, longscan, multipass, dropped, nan, dedupe, overflow, bigbin, bad = map(int, m.groups())
    assert bad == 0, "\n".join(ln for ln in report.splitlines() if not ln.endswith("mismatches 0"))[-4000:]
    assert cases >= 50 and jobs >= 70 and tiles >= 1500, m.group(0)
    # each path was taken: several tiles, a scan run longer than one tile, several column passes, drops, NaN samples,
    # repeated ranks, a capacity overflow, max_bin above a workgroup
    assert min(multitile, longscan, multipass, dropped, nan, dedupe, overflow, bigbin) > 0, m.group(0)


def test_every_pass_count_and_max_bin_ran(report):
    want = {1: 5, 2: 5, 255: 5, 256: 5, 257: 6, 65536: 6, 65537: 7}
    for ncol, p in want.items():
        lines = [ln for ln in report.splitlines() if ln.startswith("ncol/%d/" % ncol)]
        assert lines and all(int(re.search(r"passes (\d)", ln).group(1)) == p for ln in lines), (ncol, lines)
        assert qm.passes(ncol) == p
    for B in (1, 2, 3, 255, 256, 257, 4096):
        lines = [ln for ln in report.splitlines() if ln.startswith("maxbin/%d/" % B)]
        assert lines and all(int(re.search(r"bin +(\d+)", ln).group(1)) == B for ln in lines), (B, lines)


def test_every_flag_and_both_index_widths_ran(report):
    lines = report.splitlines()
    flags = {int(re.search(r"flags +(\d+)", ln).group(1)) for ln in lines if ln.startswith("flag/")}
    assert flags >= {1, 2, 4}, flags
    assert all(int(re.search(r"flags +(\d+)", ln).group(1)) & 8 for ln in lines
               if ln.startswith(("cap/one-short", "cap/far-short", "cap/none")))
    assert any(ln.startswith("cap/two-spare") and " flags  0 " in ln for ln in lines)
    assert any(ln.startswith("window/max-entries-one-short") and " flags 16 " in ln for ln in lines)
    assert any(ln.startswith("window/max-entries-exact") and " flags  0 " in ln for ln in lines)
    for group in ("count", "special", "drop", "absent", "cap", "flag"):
        for w in ("/u32 ", "/u64 "):
            assert any(ln.startswith(group + "/") and w in ln for ln in lines), (group, w)
    assert any(ln.startswith("drop/2^32+c/u64") for ln in lines)


# ------------------------------------------------------------ the model --
def _f32(*v):
    return np.array(v, dtype=np.float32).view(U32)


def _cuts(values, B):
    """One column's cuts as float32, through the whole model (one row per sample)."""
    bits = np.asarray(values, dtype=np.float32).view(U32) if not isinstance(values, np.ndarray) or \
        values.dtype != U32 else values
    n = len(bits)
    bufs = {"cut_ptr": np.full(2 + 2, SENT, U32), "cut_value": np.full(n + 2, SENT, U32), "cap": n}
    out, st = qm.make_cuts(np.arange(n + 1, dtype=U64), np.zeros(n, U32), bits, bufs, counts=(n, n, n), ncol=1,
                           max_bin=B)
    m = st[qm.N_CUTS]
    assert list(out["cut_ptr"]) == [0, m, SENT, SENT] and (out["cut_value"][m:] == SENT).all()
    assert st[qm.KEPT] == n and st[qm.FLAGS] == 0
    return out["cut_value"][:m].view(np.float32), st


def test_model_keys_order_every_float():
    b = np.array([0xFF800000, 0xFF7FFFFF, 0xBF800000, 0x80800000, 0x807FFFFF, 0x80000001, 0x80000000, 0x00000000,
                  0x00000001, 0x007FFFFF, 0x00800000, 0x3F800000, 0x7F7FFFFF, 0x7F800000], U32)
    k = qm.key_of(b).astype(np.int64)
    assert (np.diff(k) >= 0).all() and (np.diff(k) == 0).sum() == 1  # only -0.0 and +0.0 tie
    keep = b != 0x80000000
    assert (qm.unkey(qm.key_of(b[keep])) == b[keep]).all()
    assert (qm.key_of(np.array([0x7FC00000, 0xFFC00001, 0x7F800001, 0xFFFFFFFF], U32)) == qm.NAN_KEY).all()


def test_model_1024_distinct_values_give_16_bins_of_64():
    v = np.random.default_rng(1).permutation(1024).astype(np.float32) * 0.5 - 100
    cuts, st = _cuts(v, 16)
    assert len(cuts) == 16 and (np.diff(cuts) > 0).all()
    assert np.bincount(bm.search_bin(cuts, v), minlength=16).tolist() == [64] * 16


@pytest.mark.parametrize("N,B", [(256, 256), (512, 2), (96, 3), (4096, 256), (77, 1), (1000, 125)])
def test_model_distinct_values_fill_every_bin_equally(N, B):
    v = (np.random.default_rng(N + B).permutation(N).astype(np.float32) - N // 2) * 0.25
    cuts, _ = _cuts(v, B)
    assert len(cuts) == B
    assert np.bincount(bm.search_bin(cuts, v), minlength=B).tolist() == [N // B] * B


def test_model_three_distinct_values_give_three_cuts():
    v = np.array([0] * 50 + [1] * 30 + [2] * 20, np.float32)
    np.random.default_rng(2).shuffle(v)
    cuts, st = _cuts(v, 256)
    assert cuts.view(U32).tolist() == [_f32(1)[0], _f32(2)[0], _f32(2)[0] + 1]
    assert np.bincount(bm.search_bin(cuts, v), minlength=3).tolist() == [50, 30, 20]
    assert st[qm.N_CUTS] == 3 and st[qm.EMPTY_COLS] == 0 and st[qm.NAN] == 0


def test_model_float_edges():
    fmax = np.finfo(np.float32).max
    assert _cuts([fmax], 256)[0].view(U32).tolist() == [0x7F800000]            # FLT_MAX: the last cut is +inf
    assert _cuts([-np.inf], 256)[0].view(U32).tolist() == [0xFF7FFFFF]         # -inf alone: -FLT_MAX
    assert _cuts([np.inf], 256)[0].view(U32).tolist() == [0x7F800000]          # +inf stays +inf
    assert _cuts(np.array([0x80000000, 0], U32), 256)[0].view(U32).tolist() == [1]  # {-0.0, 0.0}: the smallest denormal
    # the largest negative denormal as the maximum: the cut just above it is +0.0, never -0.0
    assert _cuts(np.array([0x80000001, 0xBF800000], U32), 2)[0].view(U32).tolist() == [0x80000001, 0]
    # NaNs of both signs are no samples; a NaN next to +inf leaves +inf on top
    cuts, st = _cuts(np.array([0x7FC00001, 0xFFC12345, 0x7F800000, 0x40400000], U32), 4)
    assert cuts.view(U32).tolist() == [0x7F800000, 0x7F800000] and st[qm.NAN] == 2
    cuts, st = _cuts(np.array([0x7FC00001, 0xFFFFFFFF], U32), 4)
    assert len(cuts) == 0 and st[qm.NAN] == 2 and st[qm.EMPTY_COLS] == 1 and st[qm.KEPT] == 2


def test_model_100k_normal_samples():
    # (distinct samples: 100000 / 256 = 390.625 gives bins of 390 or 391; a float32 tie across a rank would move one)
    rng = np.random.default_rng(3)
    v = rng.permutation(np.unique(rng.standard_normal(101000).astype(np.float32)))[:100000]
    assert len(v) == 100000
    cuts, _ = _cuts(v, 256)
    assert len(cuts) == 256 and (np.diff(cuts) > 0).all()
    occ = np.bincount(bm.search_bin(cuts, v), minlength=256)
    assert occ.min() >= 390 and occ.max() <= 391


def test_model_two_columns_drops_window_capacity_and_flags():
    # "1 0:3 1:5\n0 1:4 7:1\n1 0:3 1:6\n": column 0 = {3, 3}, column 1 = {5, 4, 6}, index 7 is dropped at ncol = 3
    off, idx, val = np.array([0, 2, 4, 6], U64), np.array([0, 1, 1, 7, 0, 1], U32), _f32(3, 5, 4, 1, 3, 6)
    bufs = lambda cap: {"cut_ptr": np.full(6, SENT, U32), "cut_value": np.full(cap + 2, SENT, U32), "cap": cap}  # noqa: E731
    out, st = qm.make_cuts(off, idx, val, bufs(4), counts=(3, 6, 6), ncol=3, max_bin=4)
    nxt = lambda x: int(_f32(x)[0]) + 1  # noqa: E731
    assert list(out["cut_ptr"]) == [0, 1, 4, 4, SENT, SENT]
    # column 1: s = [4, 5, 6], t = s[0, 0, 1, 2] -> cuts 5, 6, then just above 6
    assert list(out["cut_value"]) == [nxt(3), _f32(5)[0], _f32(6)[0], nxt(6), SENT, SENT]
    assert st == [5, 1, 3, 0, 0, 4, 1, 0]
    # one cut short: cut_ptr and the status stay exact, nothing at or past the capacity is written
    out, st = qm.make_cuts(off, idx, val, bufs(3), counts=(3, 6, 6), ncol=3, max_bin=4)
    assert list(out["cut_ptr"][:4]) == [0, 1, 4, 4] and list(out["cut_value"]) == [nxt(3), _f32(5)[0], _f32(6)[0]] + [SENT] * 2
    assert st == [5, 1, 3, qm.FLAG_CAPACITY, 0, 4, 1, 0]
    # rows 1 .. 2, no value array: every sample is 1.0f
    out, st = qm.make_cuts(off, idx, None, bufs(4), counts=(3, 6, 0), ncol=2, max_bin=256, row_begin=1)
    assert list(out["cut_ptr"][:3]) == [0, 1, 2] and list(out["cut_value"][:2]) == [nxt(1), nxt(1)]
    assert st == [3, 1, 3, 0, 0, 2, 0, 0]
    # an empty window, a failed parse and a bad value count: cut_ptr all 0, cut_value untouched
    for kw, flag in ((dict(max_rows=0), 0), (dict(row_begin=3), 0), (dict(error=3), qm.FLAG_ERROR)):
        out, st = qm.make_cuts(off, idx, val, bufs(4), counts=(3, 6, 6), ncol=3, max_bin=4, **kw)
        assert list(out["cut_ptr"]) == [0, 0, 0, 0, SENT, SENT] and (out["cut_value"] == SENT).all()
        assert st == [0, 0, qm.NONE, flag, 0, 0, 3, 0]
    out, st = qm.make_cuts(off, idx, val, bufs(4), counts=(3, 6, 5), ncol=3, max_bin=4)
    assert st == [0, 0, qm.NONE, qm.FLAG_VALUE_COUNT, 0, 0, 3, 0]
    # max_entries one short of the window
    out, st = qm.make_cuts(off, idx, val, bufs(4), counts=(3, 6, 6), ncol=3, max_bin=4, max_entries=5)
    assert st[qm.FLAGS] == qm.FLAG_MAX_ENTRIES and st[qm.KEPT] == 4
