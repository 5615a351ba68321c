"""CPU runs of the float label / weight tile body of the single-pass CSV family
(csv_fast.h tile<MODE, true, 0, false>; tests/emu/emu_csv_ws.cpp, ASan) on
header rows, text, missing values, blanks and BOMs, against the oracle and the
reference's recorded results (tests/golden/csv_sp_text.json).

Every comparison is bit-exact on offset / label / weight / index / value.  The
classes of tests/fuzz_csv_sp.py that are inside the single-pass grammar by
construction must report path == "fast" for every case; the violations must
take the exact kernels; the other inputs may take either path."""
import numpy as np
import pytest

import fuzz_csv_sp as fz
import fuzz_text
from fuzz_ws import TILE
from golden_util import dec, diff, load_json
from oracle import pyoracle as po
from tests.emu import pyemu_ws

BIG = 3 * TILE + 321
FIXTURE = load_json("csv_sp_text.json")


def check_fail(h, nunits):
    import dmlc_amd
    return bool(h["error"]) or (nunits > 0 and dmlc_amd.chunk_check(h, "csv", nunits, h["counts"]) >= 0)


def emu_vs_oracle(data, offs, want_fast=None, **kw):
    """kw in pyemu_ws's names; returns the emulator's result."""
    o = po.parse_chunks(data, offs, fmt=po.CSV, **{k: v for k, v in kw.items() if k != "exact"})
    h = pyemu_ws.parse(data, offs, **kw)
    failed = check_fail(h, (len(offs) - 1) * max(kw.get("nthread", 1), 1))
    assert (o["status"] != 0) == failed, (data[:200], offs, kw, o["msg"], h["error"])
    if not failed:
        assert diff(h, o) == [], (diff(h, o), data[:200], offs, kw)
    if want_fast is not None:
        assert (h["path"] == "fast") == want_fast, (h["path"], data[:200], offs, kw)
    return h


def _fx_kw(prm):
    return {"delimiter": prm["delimiter"], "label_column": prm["label_column"], "weight_column": prm["weight_column"]}


def test_oracle_matches_reference_fixture():
    """The C restatement against what the genuine reference recorded."""
    for case in FIXTURE:
        o = po.parse_chunks(case["data_latin1"].encode("latin-1"), case["offs"], fmt=po.CSV, **_fx_kw(case["params"]))
        assert (o["status"] != 0) == bool(case["status"]), (case["name"], o["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(o, exp) == [], (case["name"], diff(o, exp))


def test_fixture_states_the_field_rule():
    """DESIGN 3.2's example, as the reference recorded it: a header word and an
    empty field at the label column are labels of 0."""
    case = {c["name"]: c for c in FIXTURE}["table_header_label0"]
    exp = {k: dec(v) for k, v in case["expect"].items()}
    assert exp["label"].tolist() == [0, 1, 0] and exp["offset"].tolist() == [0, 2, 4, 5]
    assert exp["value"].tolist() == [0, 0, 2.5, 3, 4]


@pytest.mark.parametrize("part", range(4))
def test_emu_reference_fixture(part):
    """The reference's table, the small edge cases and the violations through
    the tile bodies: its arrays, the single pass wherever it must stand and
    the exact kernels for every violation."""
    for case in FIXTURE[part::4]:
        data = case["data_latin1"].encode("latin-1")
        h = pyemu_ws.parse(data, case["offs"], **_fx_kw(case["params"]))
        failed = check_fail(h, len(case["offs"]) - 1)
        assert failed == bool(case["status"]), (case["name"], h["error"], case["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(h, exp) == [], (case["name"], diff(h, exp))
        if case["fast"]:
            assert h["path"] == "fast", case["name"]
        if case["exact"]:
            assert h["path"] == "exact", case["name"]


@pytest.mark.parametrize("form", fz.FORMS, ids=["l0", "l1", "llast", "l0w2", "l3w1"])
@pytest.mark.parametrize("cls", fz.CLASSES)
def test_emu_classes_stay_single_pass(cls, form):
    """Headers, text and missing values, blanks, BOMs: every input stays on
    the single pass and equals the oracle; small inputs, both index widths,
    nthread=3, line-aligned chunk cuts, and one input of three tiles and a bit."""
    rng = np.random.default_rng(4000 + 10 * fz.CLASSES.index(cls) + fz.FORMS.index(form))
    for it in range(6):
        data, lc, wc = fz.gen(rng, cls, int(rng.integers(1, 41)), form)
        kw = {"label_column": lc, "weight_column": wc, "index_bits": 64 if it % 3 == 1 else 32}
        if it == 4:
            kw["nthread"] = 3
        # (BOMs: one input with a chunk cut at every later row-start BOM)
        cuts = fz.bom_cuts(data) if cls == "boms" and it == 5 else fuzz_text.random_cuts(rng, data, 4)
        emu_vs_oracle(data, cuts, want_fast=True, **kw)
    data, lc, wc = fz.sized(rng, cls, form, BIG)
    assert len(data) > 3 * TILE
    emu_vs_oracle(data, fuzz_text.random_cuts(rng, data, 5), want_fast=True, label_column=lc, weight_column=wc)


def test_emu_label0_text_row_longer_than_a_tile():
    """label_column=0 alone: a field of a carried-in row is never special, so
    rows of text fields may span tiles."""
    rng = np.random.default_rng(12)
    words = ["NA", "", "?", "abc", "1.5", "x", "nan", ""]
    rows = []
    for n in (5000, 12, 9000, 3):
        rows.append(",".join(words[int(x)] for x in rng.integers(0, len(words), size=n)) + ",1")
    data = ("\n".join(rows) + "\n").encode()
    assert len(data) > 2 * TILE
    emu_vs_oracle(data, [0, len(data)], want_fast=True, label_column=0)


def test_emu_edges():
    """Tokenless special fields in a carried-in row, label fields cut by
    segment and tile boundaries, a header longer than a tile, CRLF, and a BOM
    before 61..130 blanks around a segment boundary (labelled, plain, tab)."""
    for name, data, lc, wc, delim, fast in fz.edge_cases():
        emu_vs_oracle(data, [0, len(data)], want_fast=fast, label_column=lc, weight_column=wc, delimiter=delim)


def test_emu_violations():
    """A NaN weight (one row, every row), a short row, an empty last-column
    label, a one-field row under label_column=0: the exact kernels and the
    reference's result or error -- alone, and behind an input of several tiles."""
    rng = np.random.default_rng(5)
    for name, text, lc, wc in fz.violations():
        data = text.encode("latin-1")
        emu_vs_oracle(data, [0, len(data)], want_fast=False, label_column=lc, weight_column=wc)
        ncols = text.split("\n")[0].count(",") + 1
        base = fz.sized(rng, "text", (lc, wc), TILE + 100, ncols)[0]
        big = base + data
        emu_vs_oracle(big, [0, len(base), len(big)], want_fast=False, label_column=lc, weight_column=wc)


def test_emu_ws_label_kernel_still_clean_input_only():
    """The whitespace-mode label kernel keeps its clean form: a blank after
    the delimiter still declines."""
    data = b"1\t 2\t3\n"
    emu_vs_oracle(data, [0, len(data)], want_fast=False, delimiter="\t", label_column=1)
    data = b"1\t2\t3\n"
    emu_vs_oracle(data, [0, len(data)], want_fast=True, delimiter="\t", label_column=1)


def test_emu_fast_equals_exact_chunk_table():
    rng = np.random.default_rng(8)
    data, lc, wc = fz.gen(rng, "text", 60, (3, 1), 7)
    offs = [0, data.index(b"\n", len(data) // 2) + 1, len(data)]
    hf = emu_vs_oracle(data, offs, want_fast=True, label_column=lc, weight_column=wc)
    he = emu_vs_oracle(data, offs, want_fast=False, label_column=lc, weight_column=wc, exact=True)
    assert hf["chunk_table"].tolist() == he["chunk_table"].tolist()
