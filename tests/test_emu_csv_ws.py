"""CPU runs of the single-pass CSV tile bodies for whitespace delimiters and
integer label columns (csv_fast.h tile<MODE, SP, VT, WS>; tests/emu/emu_csv_ws.cpp,
ASan) against the oracle and the reference's recorded results.

Every comparison is bit-exact on offset / label / weight / index / value.  The
classes of tests/fuzz_ws.py that are inside the single-pass grammar by
construction must report path == "fast" for every case; the others may take
either path."""
import numpy as np
import pytest

import fuzz_text
import fuzz_ws
from golden_util import dec, diff, load_json
from oracle import pyoracle as po
from tests.emu import pyemu, pyemu_ws
from tools import synth

VT = {"f32": 0, "i32": 1, "i64": 2}
DELIMS = ["\t", " "]
BIG = 3 * fuzz_ws.TILE + 321


def check_fail(h, offs):
    import dmlc_amd
    nch = len(offs) - 1
    return bool(h["error"]) or (nch > 0 and dmlc_amd.chunk_check(h, "csv", nch, h["counts"]) >= 0)


def emu_vs_oracle(data, offs, want_fast=None, emu=pyemu_ws, **kw):
    """kw in pyemu's names; returns the emulator's result."""
    okw = {("value_kind" if k == "value_type" else k): v for k, v in kw.items() if k not in ("tile_bytes", "exact")}
    nthread = kw.get("nthread", 1)
    o = po.parse_chunks(data, offs, fmt=po.CSV, **okw)
    h = emu.parse(data, offs, **kw) if emu is pyemu_ws else emu.parse(data, offs, "csv", **kw)
    failed = check_fail(h, [0] * ((len(offs) - 1) * max(nthread, 1) + 1))
    assert (o["status"] != 0) == failed, (data[:200], offs, kw, o["msg"], h["error"])
    if not failed:
        assert diff(h, o) == [], (diff(h, o), data[:200], offs, kw)
    if want_fast is not None:
        assert (h["path"] == "fast") == want_fast, (h["path"], data[:200], offs, kw)
    return h


FIXTURE = load_json("csv_ws.json")


def _fx_kw(prm):
    return {"delimiter": prm["delimiter"], "value_type": prm["value_kind"]}


def test_oracle_matches_reference_fixture():
    """The C restatement against what the genuine reference recorded."""
    for case in FIXTURE:
        prm = case["params"]
        o = po.parse_chunks(case["data_latin1"].encode("latin-1"), case["offs"], fmt=po.CSV,
                            delimiter=prm["delimiter"], value_kind=prm["value_kind"])
        assert (o["status"] != 0) == bool(case["status"]), (case["name"], o["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(o, exp) == [], (case["name"], diff(o, exp))


@pytest.mark.parametrize("part", range(4))
def test_emu_reference_fixture(part):
    """The reference's table, the small edge cases and the violations through
    the tile bodies: its arrays, and the single pass wherever it must stand."""
    for case in FIXTURE[part::4]:
        data = case["data_latin1"].encode("latin-1")
        h = pyemu_ws.parse(data, case["offs"], **_fx_kw(case["params"]))
        failed = check_fail(h, case["offs"])
        assert failed == bool(case["status"]), (case["name"], h["error"], case["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(h, exp) == [], (case["name"], diff(h, exp))
        if case["fast"]:
            assert h["path"] == "fast", case["name"]


@pytest.mark.parametrize("vt", ["f32", "i32", "i64"])
@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
@pytest.mark.parametrize("cls", ["clean", "runs"])
def test_emu_ws_classes_stay_single_pass(cls, delim, vt):
    """Classes 1 and 2: every input stays on the single pass and equals the
    oracle; small inputs, both index widths, line-aligned chunk cuts, FillData
    ranges, and one input of three tiles and a bit."""
    rng = np.random.default_rng(1000 + 10 * DELIMS.index(delim) + VT[vt] + (100 if cls == "runs" else 0))

    def gen(nlines, maxcols):
        if cls == "clean":
            return fuzz_ws.clean(rng, nlines, maxcols, delim, ints=vt != "f32")
        return fuzz_ws.runs(rng, nlines, maxcols, delim, ints=vt != "f32")

    for it in range(6):
        data = gen(int(rng.integers(1, 41)), int(rng.integers(1, 30)))
        offs = fuzz_text.random_cuts(rng, data, 4)
        kw = {"delimiter": delim, "value_type": VT[vt], "index_bits": 64 if it % 3 == 1 else 32}
        if it == 4:
            kw["nthread"] = 3
        emu_vs_oracle(data, offs, want_fast=True, **kw)
    data = fuzz_ws.sized(lambda n: gen(n, 40), BIG)
    assert len(data) > 3 * fuzz_ws.TILE
    emu_vs_oracle(data, fuzz_text.random_cuts(rng, data, 5), want_fast=True, delimiter=delim, value_type=VT[vt])


@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_emu_ws_edges(delim):
    """Class 3: blank runs across segment, tile and pre-halo boundaries (cut
    before, at and after the structural delimiter), 62 and 64+ blanks, chunk
    starts inside runs, a row over two tiles, CRLF, words, junk after blanks."""
    rng = np.random.default_rng(77 + DELIMS.index(delim))
    for name, data, offs, fast, f32_only in fuzz_ws.edge_cases(delim):
        for vt in ("f32", "i32") if len(data) < 1000 or name.endswith("split2") else ("f32",):
            if offs is None:
                cuts = [fuzz_text.random_cuts(rng, data, 6, anywhere=True) for _ in range(4)]
            else:
                cuts = [[0, len(data)] if offs == "whole" else offs]
            for c in cuts:
                want = True if fast and not (f32_only and vt != "f32") else None
                emu_vs_oracle(data, c, want_fast=want, delimiter=delim, value_type=VT[vt])


@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_emu_ws_violations(delim):
    """Class 4: outside the single-pass grammar -- the reference's result
    whichever path runs, also appended to an input of several tiles."""
    rng = np.random.default_rng(5)
    base = fuzz_ws.sized(lambda n: fuzz_ws.runs(rng, n, 20, delim), fuzz_ws.TILE + 100)
    for name, data, offs in fuzz_ws.violations(delim):
        for vt in ("f32", "i64"):
            o = offs if offs is not None else [0, len(data)]
            emu_vs_oracle(data, o, delimiter=delim, value_type=VT[vt])
        big = base + data
        emu_vs_oracle(big, [0, len(base), len(big)] if offs is None else [0] + [len(base) + x for x in offs],
                      delimiter=delim, value_type=0)


@pytest.mark.parametrize("vt", ["i32", "i64"])
@pytest.mark.parametrize("delim", [",", "\t"], ids=["comma", "tab"])
def test_emu_int_label_column(delim, vt):
    """Class 5: integer DTypes with a label column (stored as the DType,
    decoded by strtoll): label first, second and last, an ordinary
    weight_column in some, one input of several tiles; every clean input
    stays on the single pass.  An empty label field and a one-field row under
    label_column=0 (the reference's fatal error) go to the exact kernels."""
    rng = np.random.default_rng(300 + VT[vt] + (10 if delim == "\t" else 0))
    ncols = 7
    for it, lc in enumerate((0, 1, ncols - 1, 0, 1, ncols - 1)):
        data = fuzz_text.labeled_csv(rng, int(rng.integers(1, 41)), ncols, lc, delim)
        kw = {"delimiter": delim, "value_type": VT[vt], "label_column": lc, "index_bits": 64 if it == 2 else 32}
        if it >= 3:
            kw["weight_column"] = (2, 0, 3)[it - 3]  # an ordinary column for integer DTypes
        if it == 5:
            kw["nthread"] = 3
        h = emu_vs_oracle(data, fuzz_text.random_cuts(rng, data, 4), want_fast=True, **kw)
        assert h["label"].dtype == (np.int32 if vt == "i32" else np.int64) and len(h["label"]) == len(h["offset"]) - 1
    data = fuzz_ws.sized(lambda n: fuzz_text.labeled_csv(rng, n, 12, 0, delim), BIG)
    emu_vs_oracle(data, fuzz_text.random_cuts(rng, data, 5), want_fast=True, delimiter=delim, value_type=VT[vt],
                  label_column=0)
    for kind, lc in (("empty", 0), ("empty", 2), ("one_field", 0)):
        data = fuzz_ws.int_label_defect(rng, 12, ncols, lc, kind, delim)
        o = po.parse_chunks(data, [0, len(data)], fmt=po.CSV, delimiter=delim, value_kind=VT[vt], label_column=lc)
        assert (o["status"] != 0) == (kind == "one_field"), o["msg"]  # "Delimiter not found" must be raised
        emu_vs_oracle(data, [0, len(data)], want_fast=False, delimiter=delim, value_type=VT[vt], label_column=lc)


def test_emu_float_label_weight_columns_tab():
    """Class 6: the label / weight kernel with '\\t': clean inputs stay on the
    single pass; a doubled delimiter is outside its clean form and declines."""
    rng = np.random.default_rng(66)
    for it, (lc, wc) in enumerate(((0, -1), (2, -1), (-1, 1), (0, 2), (3, 1), (1, 4))):
        ncols = max(lc, wc) + 2 + int(rng.integers(0, 6))
        big = it == 3
        data = fuzz_text.labeled_csv(rng, 40, ncols, lc, "\t", weight_col=wc) if not big else fuzz_ws.sized(
            lambda n: fuzz_text.labeled_csv(rng, n, ncols, lc, "\t", weight_col=wc), BIG)
        kw = {"delimiter": "\t", "label_column": lc, "weight_column": wc}
        emu_vs_oracle(data, fuzz_text.random_cuts(rng, data, 4), want_fast=True, **kw)
        if not big:
            emu_vs_oracle(fuzz_ws.doubled(data, "\t", rng), [0, len(data) + 1], want_fast=False, **kw)
    # a delimiter at a row start, a trailing delimiter, the other blank: not clean either
    for text in ("\t1\t2\t3\n", "1\t2\t3\t\n4\t5\t6\n", "1\t 2\t3\n"):
        emu_vs_oracle(text.encode(), [0, len(text)], want_fast=False, delimiter="\t", label_column=1)


def test_old_emulator_driver_keeps_its_exact_path():
    """tests/emu/emu.cpp decides with csv_fast_int_ok / csv_fast_columns_ok and
    its own delimiter rule, and runs the plain integer tile body for every
    integer input: those predicates kept their meaning, so it still sends a
    whitespace delimiter and an integer label column to the exact kernels and
    its result is still the reference's."""
    rng = np.random.default_rng(9)
    data = fuzz_ws.clean(rng, 30, 12, "\t")
    emu_vs_oracle(data, [0, len(data)], want_fast=False, emu=pyemu, delimiter="\t")
    data = fuzz_text.labeled_csv(rng, 30, 6, 0)
    emu_vs_oracle(data, [0, len(data)], want_fast=False, emu=pyemu, value_type=1, label_column=0)


@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_emu_ws_fast_equals_exact_synthetic(delim):
    text, _ = synth.rows(synth.CSV, 150, 24, seed=3)
    data = fuzz_ws.with_delim(text.tobytes(), delim)
    offs = [0, data.index(b"\n", len(data) // 2) + 1, len(data)]
    hf = emu_vs_oracle(data, offs, want_fast=True, delimiter=delim)
    he = emu_vs_oracle(data, offs, want_fast=False, delimiter=delim, exact=True)
    assert hf["chunk_table"].tolist() == he["chunk_table"].tolist()
