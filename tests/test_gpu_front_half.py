"""GPU parity for the single-pass front half of interior tiles (svm_fast.h
front_half / front_commit: classification from the staging registers, the quad
exchange, the tail by ballots, the "qid:" checks after the barrier).

dmlc_amd.parse_bytes against oracle.pyoracle.parse_chunks on texts of three
full tiles plus a remainder (about 55 KB): tiles 1 and 2 are interior and take
the new path, tile 0 and the last tile the old one.  Lines are padded with
blanks so that each feature lands on the byte the case names.  Every output
array equals the oracle's and error is 0; the path is the single pass wherever
the text is in the grammar.  Texts with bytes outside it (a letter, a byte >=
0x80, '#', a stray 'q', "qid:" in libfm) take the path the parent commit's
library took on the same text -- it equalled the oracle there -- recorded below
as constants."""
import numpy as np
import pytest

from golden_util import diff
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

PO_FMT = {"libsvm": po.LIBSVM, "libfm": po.LIBFM}


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


class Text:
    """Lines appended one by one; goto(p) pads the line before with blanks so that the next one starts at p."""

    def __init__(self, fmt, qid, seed):
        self.fmt, self.qid, self.rng = fmt, qid, np.random.RandomState(seed)
        self.parts, self.n, self.row = [], 0, 0

    def pairs(self, k):
        r = self.rng
        if self.fmt == "libfm":
            return " ".join("%d:%d:%s" % (r.randint(0, 30), r.randint(1, 5000), self.num()) for _ in range(k))
        return " ".join("%d:%s" % (r.randint(1, 5000), self.num()) for _ in range(k))

    def num(self):
        r = self.rng
        return ("%d" % r.randint(0, 100), "%.3f" % r.rand(), "-%.5f" % (r.rand() * 50), "%d.%d" % (r.randint(0, 9), r.randint(0, 99)))[
            r.randint(0, 4)]

    def head(self):
        self.row += 1
        return "%d" % (self.row % 2) + (" qid:%d" % (self.row // 4 + 1) if self.qid else "")

    def line(self):
        return ("%s %s\n" % (self.head(), self.pairs(int(self.rng.randint(3, 9))))).encode()

    def add(self, b):
        self.parts.append(b)
        self.n += len(b)

    def goto(self, target):
        assert self.parts and target >= self.n, (target, self.n)
        while True:
            ln = self.line()
            if self.n + len(ln) > target:
                self.row -= 1
                break
            self.add(ln)
        pad = target - self.n
        if pad:
            last = self.parts.pop()
            self.n -= len(last)
            end = b"\r\n" if last.endswith(b"\r\n") else b"\n"
            self.add(last[:-len(end)] + b" " * pad + end)
        assert self.n == target

    def fill(self, total):
        while self.n < total:
            self.add(self.line())
        return b"".join(self.parts)


def run(dm, fmt, data, want_path):
    tile, _ = dm.fast_geometry()
    assert 3 * tile + 1024 < len(data) < 4 * tile  # tiles 1 and 2 interior, a remainder after tile 2
    offs = [0, len(data)]
    o = po.parse_chunks(data, offs, fmt=PO_FMT[fmt])
    assert o["status"] == 0, o["msg"]
    h = dm.parse_bytes(data, offs, fmt=fmt)
    print("path %s want %s (%s, %d bytes)" % (h["path"], want_path, fmt, len(data)))
    assert h["error"] == 0
    assert diff(h, o) == [], (diff(h, o), fmt)
    assert h["path"] == want_path, (h["path"], want_path)
    return h


def total_of(tile):
    return 3 * tile + 6000


def qid_text(fmt, tile, stray=False):
    """"qid:" tokens whose 'q' sits at segment offsets 60, 61, 62, 63, 0 and unit offsets 13, 14, 15, 16 of
    tiles 1 and 2, and one with its letters at the end of tile 1 and its ':' and digits in tile 2."""
    t = Text(fmt, True, 11)
    t.add(t.line())
    spots = []
    for k in (1, 2):
        spots += [k * tile + 64 * (10 + 10 * i) + off for i, off in enumerate((60, 61, 62, 63, 0, 13, 14, 15, 16))]
    spots.append(2 * tile - 3)
    for p in sorted(spots):
        t.goto(p - 2)  # "<label> qid:": the 'q' two bytes into the line
        ln = t.line()
        assert ln[2:6] == b"qid:"
        t.add(ln)
        if stray and p == tile + 64 * 20 + 61:  # a 'q' alone, as a pair's neighbour in the next line
            t.add(b"%s q %s\n" % (t.head().encode(), t.pairs(3).encode()))
    data = t.fill(total_of(tile))
    for p in spots:
        assert data[p:p + 4] == b"qid:" and data[p - 2:p - 1] in (b"0", b"1"), p
    return data


def number_text(fmt, tile):
    """A value that starts in the last 15 bytes of tile 1, and one of tile 2, and continues into the next tile."""
    t = Text(fmt, False, 12)
    t.add(t.line())
    for p, num in ((2 * tile - 7, b"3.14159265"), (3 * tile - 12, b"-271.8281828459")):
        lead = b"1 4:7:" if fmt == "libfm" else b"1 7:"
        t.goto(p - len(lead))
        t.add(lead + num + b" " + t.pairs(2).encode() + b"\n")
    data = t.fill(total_of(tile))
    assert data[2 * tile - 7:2 * tile + 3] == b"3.14159265" and data[3 * tile - 12:3 * tile + 3] == b"-271.8281828459"
    return data


def crlf_text(fmt, tile):
    """"\\r\\n" line ends with the '\\r' last in a unit, last in a segment and last in tile 1 and tile 2."""
    t = Text(fmt, False, 13)
    t.add(t.line())
    ends = [tile + 64 * 9 + 15, tile + 64 * 33 + 63, 2 * tile - 1, 2 * tile + 64 * 7 + 47, 2 * tile + 64 * 100 + 63,
            3 * tile - 1]
    for p in ends:
        body = ("%s %s" % (t.head(), t.pairs(2))).encode()
        t.goto(p - len(body))
        t.add(body + b"\r\n")
    data = t.fill(total_of(tile))
    for p in ends:
        assert data[p:p + 2] == b"\r\n", p
    return data


TEXTS = {"qid": qid_text, "number": number_text, "crlf": crlf_text}
# "qid:" is no token of libfm: the letters leave its grammar
CLEAN_PATH = {("libsvm", "qid"): "fast", ("libsvm", "number"): "fast", ("libsvm", "crlf"): "fast",
              ("libfm", "qid"): "exact", ("libfm", "number"): "fast", ("libfm", "crlf"): "fast"}


@pytest.mark.parametrize("fmt", ["libsvm", "libfm"])
@pytest.mark.parametrize("case", ["qid", "number", "crlf"])
def test_features_at_unit_segment_and_tile_ends(dm, fmt, case):
    tile, _ = dm.fast_geometry()
    run(dm, fmt, TEXTS[case](fmt, tile), CLEAN_PATH[fmt, case])


def test_stray_q(dm):
    """One 'q' that belongs to no token: a byte outside the grammar (front_commit's stray)."""
    tile, _ = dm.fast_geometry()
    run(dm, "libsvm", qid_text("libsvm", tile, stray=True), STRAY_PATH)


def outside_text(tile, byte, where):
    """Lines "<label> <pairs> X <pairs>" with the byte X at chosen places."""
    t = Text("libsvm", False, 14)
    t.add(t.line())
    if where == "prehalo":  # only in the last 64 bytes of tile 1: tile 2 meets it in its pre-halo alone
        spots = [2 * tile - 30]
    elif where == "unit_ends":  # the last byte of a unit, of a segment, of tile 1; the first of a segment and of a unit
        spots = [tile + 64 * 12 + 15, tile + 64 * 40 + 63, 2 * tile - 1, 2 * tile + 64 * 3, 2 * tile + 64 * 50 + 16,
                 2 * tile + 64 * 90 + 47]
    else:  # nseg: exactly two segments of tile 1 and exactly three of tile 2 hold such a byte
        spots = [tile + 64 * 30 + 20, tile + 64 * 33 + 5, 2 * tile + 64 * 60 + 7, 2 * tile + 64 * 63 + 50,
                 2 * tile + 64 * 200 + 33]
    for p in spots:
        lead = ("%s %s " % (t.head(), t.pairs(1))).encode()
        t.goto(p - len(lead))
        t.add(lead + byte + b" " + t.pairs(2).encode() + b"\n")
    data = t.fill(total_of(tile))
    for p in spots:
        assert data[p:p + 1] == byte, p
    assert data.count(byte) == len(spots)
    return data


# the parent commit's path on these texts (its arrays equalled the oracle's)
STRAY_PATH = "exact"
OUTSIDE_PATH = {(b, w): "fast" for b in ("letter", "high", "hash") for w in ("prehalo", "unit_ends", "nseg")}
BYTES = {"letter": b"a", "high": b"\xc3", "hash": b"#"}


@pytest.mark.parametrize("kind", sorted(BYTES))
@pytest.mark.parametrize("where", ["prehalo", "unit_ends", "nseg"])
def test_bytes_outside_the_grammar(dm, kind, where):
    tile, _ = dm.fast_geometry()
    run(dm, "libsvm", outside_text(tile, BYTES[kind], where), OUTSIDE_PATH[kind, where])
