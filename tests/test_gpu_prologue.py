"""GPU parity for the single-pass tile prologue (fast_common.h: the one-trip
chunk list chunk_guess_begin / chunk_guess_end, the computed decoder tables)
in the libsvm, CSV and libfm kernels.

dmlc_amd.parse_bytes against oracle.pyoracle.parse_chunks on synthetic texts
of about 20 single-pass tiles (tools/synth) cut into ParseBlock units at line
starts by the unit-start tables of tests/test_emu_chunk_guess.py: 1, 2, 63,
64, 65, 257 and about 5000 units (the last on a longer text: a tile takes
kMaxCs starts), equal units, one unit of 90 % of the text before tiny ones, a
tile holding exactly kMaxCs one-line units and one holding kMaxCs + 1, unit
starts at tlo - 1 / tlo / thi - 1 / thi, a found unit in the window's last
lanes.  Every output array equals the oracle's, error is 0, and the path is
the single pass -- except with kMaxCs + 1 starts in a tile, which must reach
the exact kernels and still equal the oracle.  One libsvm case of fractions
and integer parts of every length across a tile end reads every entry of the
decoder tables the device computes."""
import numpy as np
import pytest

from golden_util import diff
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

FMT = {"libsvm": (synth.LIBSVM, po.LIBSVM, 12), "csv": (synth.CSV, po.CSV, 16), "libfm": (synth.LIBFM, po.LIBFM, 8)}


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


_LINES = {}


def lines_of(fmt, ntiles, tile):
    """The lines (bytes, each ending in a newline) of a synthetic text of about ntiles tiles."""
    key = (fmt, ntiles)
    if key not in _LINES:
        kind, _, width = FMT[fmt]
        probe, _ = synth.rows(kind, 64, width, seed=5)
        nrows = int(ntiles * tile / (probe.size / 64.0)) + 1
        text, offs = synth.rows(kind, nrows, width, seed=5, line_offsets=True)
        raw = text.tobytes()
        _LINES[key] = [raw[int(offs[i]):int(offs[i + 1])] for i in range(nrows)]
    return list(_LINES[key])


def pad_line(fmt, line, k):
    """`line` made k bytes longer inside the single-pass grammar: blanks before the newline (libsvm, libfm),
    extra ",0" / ",00" fields (CSV; k >= 2)."""
    if k == 0:
        return line
    if fmt != "csv":
        return line[:-1] + b" " * k + b"\n"
    assert k >= 2
    return line[:-1] + b",0" * ((k - 3) // 2 if k % 2 else k // 2) + (b",00" if k % 2 else b"") + b"\n"


def align(fmt, lines, positions):
    """Pad lines so that a line starts at each of `positions` (ascending, a tile or more apart)."""
    for pos in positions:
        starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
        j = int(np.searchsorted(starts, pos, side="right")) - 1  # last line starting at or before pos
        if fmt == "csv" and pos - starts[j] == 1:
            j -= 1
        assert j >= 1
        lines[j - 1] = pad_line(fmt, lines[j - 1], int(pos - starts[j]))
    return lines


def starts_of(lines):
    return np.concatenate([[0], np.cumsum([len(x) for x in lines])]).astype(np.int64)


def snap(ls, targets):
    """Line starts at or after each target (inside the text), ascending and distinct, 0 first."""
    idx = np.searchsorted(ls[:-1], np.asarray(targets, dtype=np.int64))
    idx = idx[idx < len(ls) - 1]
    return np.unique(np.concatenate([[0], ls[idx]]))


def run(dm, fmt, lines, units, want_fast=True):
    data = b"".join(lines)
    offs = [int(x) for x in units] + [len(data)]
    assert offs[0] == 0 and all(a < b for a, b in zip(offs, offs[1:]))
    o = po.parse_chunks(data, offs, fmt=FMT[fmt][1])
    assert o["status"] == 0, o["msg"]
    h = dm.parse_bytes(data, offs, fmt=fmt)
    assert h["error"] == 0
    assert dm.chunk_check(h, fmt, len(offs) - 1, h["counts"]) < 0
    assert diff(h, o) == [], (diff(h, o), fmt, len(offs) - 1)
    assert (h["path"] == "fast") == want_fast, (h["path"], fmt, len(offs) - 1)
    return h


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("nchunk", [1, 2, 63, 64, 65, 257, 5000])
def test_equal_units(dm, fmt, nchunk):
    tile, kmax = dm.fast_geometry()
    # about 5000 units need a longer text: at most kmax starts per tile, here about 20
    ntiles = 20 if nchunk <= 257 else 250
    lines = lines_of(fmt, ntiles, tile)
    ls = starts_of(lines)
    units = snap(ls, [ls[-1] * i // nchunk for i in range(1, nchunk)])
    assert len(units) >= nchunk * 9 // 10
    run(dm, fmt, lines, units)


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_one_big_unit_then_tiny_ones(dm, fmt):
    """The estimate misses by more than a window: the search takes over."""
    tile, kmax = dm.fast_geometry()
    lines = lines_of(fmt, 40, tile)
    ls = starts_of(lines)
    n = int(ls[-1])
    big = n // 10 * 9
    units = snap(ls, [big + (n - big) * i // 70 for i in range(70)])
    assert len(units) >= 65
    run(dm, fmt, lines, units)


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("over", [0, 1])
def test_one_line_units_fill_a_tile(dm, fmt, over):
    """Exactly kMaxCs starts in a tile stay on the single pass; kMaxCs + 1 reach the exact kernels."""
    tile, kmax = dm.fast_geometry()
    lines = lines_of(fmt, 20, tile)
    ls = starts_of(lines)
    first = int(np.searchsorted(ls, 5 * tile + 1))
    cnt = kmax + over
    assert ls[first + cnt - 1] < 6 * tile  # the run of one-line units lies inside tile 5
    coarse = [int(x) for x in snap(ls, [ls[-1] * i // 70 for i in range(1, 70)])
              if not 5 * tile <= x <= 6 * tile]
    units = np.unique(np.concatenate([coarse, ls[first:first + cnt]]))
    inside = int(((units >= 5 * tile) & (units <= 6 * tile)).sum())
    assert inside == cnt
    run(dm, fmt, lines, units, want_fast=not over)


@pytest.mark.parametrize("fmt", sorted(FMT))
@pytest.mark.parametrize("nchunk", [5, 70])
def test_unit_starts_at_tile_edges(dm, fmt, nchunk):
    """Unit starts at tlo - 1, tlo, thi - 1 and thi of a tile (line starts there, by padding the line before)."""
    tile, kmax = dm.fast_geometry()
    edges = [3 * tile - 1, 6 * tile, 10 * tile - 1, 13 * tile]  # tlo - 1 of tile 3, tlo of 6, thi - 1 of 9, thi of 12
    lines = align(fmt, lines_of(fmt, 20, tile), edges)
    ls = starts_of(lines)
    assert all(e in ls for e in edges)
    units = np.unique(np.concatenate([snap(ls, [ls[-1] * i // (nchunk - 4) for i in range(1, nchunk - 4)]), edges]))
    run(dm, fmt, lines, units)


@pytest.mark.parametrize("fmt", sorted(FMT))
def test_found_unit_in_the_last_lanes(dm, fmt):
    """60 units: the whole table is one window, and past unit 30 the list may leave it -- the reload."""
    tile, kmax = dm.fast_geometry()
    lines = lines_of(fmt, 20, tile)
    ls = starts_of(lines)
    units = snap(ls, [ls[-1] * i // 60 for i in range(1, 60)])
    assert len(units) >= 55
    run(dm, fmt, lines, units)


def test_every_decoder_table_entry(dm):
    """Fractions of 1-15 digits after integer parts of 0-14 digits, with and without a sign, across a tile end:
    the '.' sits at every window byte, so every p10 / i10 / hib entry the device computed is read."""
    tile, kmax = dm.fast_geometry()
    rng = np.random.RandomState(7)

    def digits(k):
        return "".join(str(d) for d in rng.randint(0, 10, size=k))

    vals = []
    for rep in range(3):
        for il in range(0, 15):
            for fl in range(1, 16):
                for sign in ("", "-", "+"):
                    ip = (str(rng.randint(1, 10)) + digits(il - 1)) if il else ""
                    vals.append("%s%s.%s" % (sign, ip, digits(fl)))
    order = rng.permutation(len(vals))
    lines, row = [], []
    for j, i in enumerate(order):
        row.append("%d:%s" % (j % 1000 + 1, vals[i]))
        if len(row) == 9:
            lines.append(("%d %s\n" % (j % 2, " ".join(row))).encode())
            row = []
    data = b"".join(lines)
    assert len(data) > 2 * tile
    ls = starts_of(lines)
    run(dm, "libsvm", lines, snap(ls, [len(data) // 3]))
