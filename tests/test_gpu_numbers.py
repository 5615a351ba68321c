"""Number decoding on the device at every decoder's numeric edges.

The catalogue of tests/numcat.py -- every fraction of 1-5 digits, decimals on
either side of f32 rounding midpoints, integer parts around every power of two
and ten, exponents across the float range, malformed numbers, lengths on both
sides of the 16-byte window's accept / decline edge, inf / nan literals,
strtoll's prefixes and saturation -- goes through the tile kernels of
libsvm.hip, csv.hip and libfm.hip in every numeric role, on the single pass
and with FLAG_EXACT, at every alignment to a thread's 64-byte segment, across
tile ends, chunk ends and the end of the text, through the lean libsvm kernel,
and through dmlc_amd_strtof_batch.  Expected arrays come from the oracle, which
tests/test_numcat.py pins on these very strings to the recorded genuine
reference and to an exact-arithmetic model; everything is bit for bit, through
full calls with guard bands (tests/full_call.py).

Every test prints what it placed and which path each input took (pytest -s);
DESIGN.md section 4 has the figures of one run and the mutations tried.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_call as fc
import numcases as nc
import numcat
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

FMTS = [po.LIBSVM, po.CSV, po.LIBFM]
IDS = ["libsvm", "csv", "libfm"]


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


@pytest.fixture(scope="module")
def dense():
    return {c["fmt"]: c for c in nc.dense_cases()}


@pytest.fixture(scope="module")
def roles():
    return nc.role_cases()


def _run_all(dm, cases, exact=False):
    """Every case, all failures reported together; returns (stayed, handed, raised)."""
    bad, stay, hand, raised = [], 0, 0, 0
    for c in cases:
        try:
            h = nc.run_case(dm, fc, c, exact=exact)
            c["took"] = "raised" if h["error"] else "single pass" if h["path"] == 0 else "handed over"
            stay += h["path"] == 0 and not h["error"]
            hand += h["path"] != 0 and not h["error"]
            raised += bool(h["error"])
        except AssertionError as e:
            bad.append(str(e)[:700])
    assert bad == [], "\n".join(bad)
    return stay, hand, raised


def _report(what, cases, counts):
    print("%s: %d inputs, %d numbers (%d window, %d byte); %d single-pass, %d handed over, %d raised"
          % (what, len(cases), sum(c["numbers"] for c in cases), sum(c["window"] for c in cases),
             sum(c["byte"] for c in cases), counts[0], counts[1], counts[2]))


# ------------------------------------------------------ value role, dense --
@pytest.mark.parametrize("exact", [False, True], ids=["single_pass", "exact"])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_gpu_dense_values(dm, dense, fmt, exact):
    """Every 1-5 digit fraction under three heads and the 64 000 midpoint
    neighbours as values, 8 per row: all decoded by the window form, on the
    single pass (path == 0) and in the exact kernels (FLAG_EXACT)."""
    c = dense[fmt]
    assert c["numbers"] == 3 * 111110 + 64000 and c["byte"] == 0
    _report("dense %s %s" % (IDS[FMTS.index(fmt)], "exact" if exact else "single pass"), [c], _run_all(dm, [c], exact))


# -------------------------------------------------- every role, compact set --
@pytest.mark.parametrize("exact", [False, True], ids=["single_pass", "exact"])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_gpu_every_role(dm, roles, fmt, exact):
    """The compact catalogue in each numeric role of the format.  Per role the
    entries inside the kernel's grammar stay on the single pass; the rest is
    handed over or raises exactly as the oracle does."""
    cases = [c for c in roles if c["fmt"] == fmt]
    assert len(cases) >= 12
    ins = [c for c in cases if c["name"].endswith("/in")]
    assert all(c["expect"] == "stay" and c["parsed"] for c in ins)
    for c in ins:  # no role went hollow: both decoder forms are in every one
        assert c["window"] >= 5 and c["byte"] >= 5, (c["name"], c["window"], c["byte"])
    counts = _run_all(dm, cases, exact)
    _report("roles %s %s" % (IDS[FMTS.index(fmt)], "exact" if exact else "single pass"), cases, counts)
    if not exact:
        assert counts[0] >= len(ins) and counts[1] + counts[2] >= 2, counts
        for c in cases:
            print("  %-40s numbers %5d window %5d byte %5d: %s" % (c["name"], c["numbers"], c["window"], c["byte"],
                                                                   c["took"]))


# ------------------------------------------------------------- alignment --
def _residues_ok(data, entries, starts):
    for s, st in zip(entries, starts):
        assert {x % 64 for x in st} == set(range(64)), s
        for x in st:
            assert data[x:x + len(s)] == s.encode("latin-1"), (s, x)


@pytest.mark.parametrize("fmt", [po.LIBSVM, po.CSV], ids=["libsvm", "csv"])
def test_gpu_alignment_sweep(dm, fmt):
    """The boundary and degenerate classes and 200 midpoint neighbours with
    their first byte at every offset 0..63 of a thread's 64-byte segment."""
    build = nc.align_svm if fmt == po.LIBSVM else nc.align_csv
    c, entries, starts = build(nc.sweep_entries())
    assert len(entries) >= 440
    _residues_ok(c["data"], entries, starts)
    _report("alignment " + c["name"], [c], _run_all(dm, [c]))
    _run_all(dm, [c], exact=True)


@pytest.mark.parametrize("half", [0, 1])
@pytest.mark.parametrize("fmt", [po.LIBSVM, po.CSV], ids=["libsvm", "csv"])
def test_gpu_numbers_across_tile_ends(dm, fmt, half):
    """The same entries with their first byte in the last 15 bytes of a tile
    (one tile per entry, so the sweep's entries go in two texts of half each)."""
    tile = dm.fast_geometry()[0]
    build = nc.tile_end_svm if fmt == po.LIBSVM else nc.tile_end_csv
    every = nc.sweep_entries()
    c, entries, starts = build(every[half::2], tile)
    assert len(every) >= 460 and len(entries) >= 220
    for i, (s, x) in enumerate(zip(entries, starts)):
        assert c["data"][x:x + len(s)] == s.encode("latin-1")
        assert 1 <= (i + 1) * tile - x <= 15 and x // tile == i
    assert {(i + 1) * tile - x for i, x in enumerate(starts)} == set(range(1, 16))
    _report("tile ends %s half %d" % (c["name"], half), [c], _run_all(dm, [c]))


def test_gpu_numbers_before_chunk_starts(dm):
    """Entries that end within 15 bytes before a chunk start of a multi-chunk
    call: the 16-byte window would pass its chunk, the byte decoder takes over."""
    cases = nc.chunk_end_cases(nc.sweep_entries(), *dm.fast_geometry())
    for c in cases:
        assert len(c["offs"]) >= 440
        cs = np.asarray(c["offs"])
        near = sum(1 for e in c["ends"] if 0 < cs[np.searchsorted(cs, e, side="right")] - e <= 15)
        assert near >= 440, (c["name"], near)
    _report("chunk ends", cases, _run_all(dm, cases))
    _run_all(dm, cases, exact=True)


def test_gpu_numbers_at_the_end_of_the_text(dm):
    """The same entries as the last bytes of a text, with and without a final newline."""
    cases = nc.text_end_cases(nc.sweep_entries())
    assert len(cases) >= 4 * 440
    _report("text end", cases, _run_all(dm, cases))


# --------------------------------------------------------- strtof_batch --
def test_gpu_strtof_batch_numcat(dm):
    """tests/golden/numcat.npz (recorded from the genuine reference) through
    dmlc_amd_strtof_batch: values and bytes consumed."""
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "numcat.npz"))
    strs = z["text"].tobytes().decode("latin-1").split("\0")
    v, n, bad = dm.strtof_batch(strs)
    got = v.view(np.uint32)
    mism = np.nonzero((got != z["bits"]) | (n != z["used"]))[0]
    assert len(mism) == 0, [(strs[i], hex(z["bits"][i]), hex(got[i]), z["used"][i], n[i]) for i in mism[:10]]
    assert not bad.any()
    v, n, bad = dm.strtof_batch(list(numcat.RAISES))
    assert bad.all()  # the unclosed "nan(" literals: flagged, as the reference's fatal check


# ---------------------------------------------------------- lean kernel --
def test_gpu_numbers_lean_kernel(dm):
    """The libsvm dense input and compact roles through svm_lean_tile: a fresh
    child process (tests/numbers_child.py) with DMLC_AMD_LEAN=1.  The clustered
    many-chunks input proves the launch (path == 0 only under the lean
    kernel, as tests/test_gpu_full_call.py).  The last test of this file; a
    child that is killed by a signal, aborts or runs out of time ends the
    whole session: nothing more may start on a GPU after that."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    try:
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "numbers_child.py")], capture_output=True,
                           timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/numbers_child.py hung on the GPU: nothing more is started there", returncode=3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit("tests/numbers_child.py died (%d) on the GPU: nothing more is started there\n%s"
                    % (r.returncode, r.stderr.decode()[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert [c for c in out["cases"] if not c["ok"]] == []
    assert len(out["cases"]) >= 20
    assert out["cluster_path"] == 0, out["cluster_path"]
    stay = sum(c["path"] == 0 and not c["error"] for c in out["cases"])
    print("lean child: %d inputs, %d numbers, %d stayed single-pass" % (len(out["cases"]),
                                                                         sum(c["numbers"] for c in out["cases"]), stay))
