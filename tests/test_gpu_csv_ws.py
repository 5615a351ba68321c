"""GPU parity for the single-pass CSV kernels' whitespace-delimiter mode and
integer label form (csv_fast.h tile<MODE, SP, VT, WS>; csv.hip
csv_fast_tile_ws / _int_ws / _sp_ws / _int_sp / _int_sp_ws).

Through the C ABI (dmlc_amd.parse_bytes) as tests/test_gpu_parity.py does, and
through the C++ Parser.  Every comparison is bit-exact on offset / label /
weight / index / value against the oracle or the reference's recorded arrays;
the classes of tests/fuzz_ws.py that are inside the single-pass grammar by
construction must report path == "fast" for every case."""
import numpy as np
import pytest

import fuzz_text
import fuzz_ws
from golden_util import dec, diff, load_json
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

VT = {"f32": 0, "i32": 1, "i64": 2}
DELIMS = ["\t", " "]
BIG = 3 * fuzz_ws.TILE + 321


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def gpu_parse(dm, data, chunk_offsets=None, **kw):
    h = dm.parse_bytes(data, chunk_offsets, fmt="csv", **kw)
    nch = (len(chunk_offsets) - 1) if chunk_offsets is not None else (1 if len(data) else 0)
    nch *= h["units_per_chunk"]
    failed = nch > 0 and dm.chunk_check(h, "csv", nch, h["counts"]) >= 0
    h["failed"] = bool(h["error"]) or failed
    return h


def _oracle_vs_gpu(dm, data, offs, want_fast=None, **kw):
    okw = {("value_kind" if k == "value_type" else k): v for k, v in kw.items() if k not in ("tile_bytes", "exact")}
    o = po.parse_chunks(data, offs, fmt=po.CSV, **okw)
    h = gpu_parse(dm, data, offs, **kw)
    assert (o["status"] != 0) == h["failed"], (o["msg"], h["error"], data[:200], offs, kw)
    if o["status"] == 0:
        bad = diff(h, o)
        assert bad == [], (bad, data[:200], offs, kw)
    if want_fast is not None:
        assert (h["path"] == "fast") == want_fast, (h["path"], data[:200], offs, kw)
    return h


def _both_paths(dm, data, offs, want_fast=None, **kw):
    """The default path and the forced exact path both equal the oracle."""
    h = _oracle_vs_gpu(dm, data, offs, want_fast=want_fast, **kw)
    he = _oracle_vs_gpu(dm, data, offs, want_fast=False, exact=True, **kw)
    if not h["failed"]:
        assert h["chunk_table"].tolist() == he["chunk_table"].tolist()
    return h


def _count_only_equals_full(dm, data, offs, **kw):
    """The size query alone (COUNT_ONLY) against the one-call pipeline's totals."""
    import torch
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    p = dm.DeviceParser("csv", **kw)
    counts = [int(x) for x in p.count(text, cs)[:8]]
    out = p.alloc(counts)
    res = torch.zeros(16, dtype=torch.int64, device="cuda")
    p.parse_into(text, cs, out, res)
    r = res.cpu().numpy().view(np.uint64)
    assert int(r[8]) == 0 and [int(x) for x in r[:8]] == counts, (counts, r[:10])
    return int(r[9])  # path of the full call: 0 = single pass


FIXTURE = load_json("csv_ws.json")


def test_gpu_reference_fixture(dm):
    """What the genuine reference recorded for the whitespace table, the small
    edge cases and the violations; the single pass wherever it must stand."""
    for case in FIXTURE:
        prm = case["params"]
        h = gpu_parse(dm, case["data_latin1"].encode("latin-1"), case["offs"], delimiter=prm["delimiter"],
                      value_type=prm["value_kind"])
        assert h["failed"] == bool(case["status"]), (case["name"], h["error"], case["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(h, exp) == [], (case["name"], diff(h, exp))
        if case["fast"]:
            assert h["path"] == "fast", case["name"]


@pytest.mark.parametrize("vt", ["f32", "i32", "i64"])
@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
@pytest.mark.parametrize("cls", ["clean", "runs"])
def test_gpu_ws_classes_stay_single_pass(dm, cls, delim, vt):
    """Classes 1 and 2 on the default path (always the single pass) and with
    exact=True; one input of three tiles and a bit; count_only on one case."""
    rng = np.random.default_rng(2000 + 10 * DELIMS.index(delim) + VT[vt] + (100 if cls == "runs" else 0))

    def gen(nlines, maxcols):
        if cls == "clean":
            return fuzz_ws.clean(rng, nlines, maxcols, delim, ints=vt != "f32")
        return fuzz_ws.runs(rng, nlines, maxcols, delim, ints=vt != "f32")

    for it in range(8):
        data = gen(int(rng.integers(1, 41)), int(rng.integers(1, 30)))
        offs = fuzz_text.random_cuts(rng, data, 4)
        kw = {"delimiter": delim, "value_type": VT[vt], "index_bits": 64 if it % 3 == 1 else 32}
        if it == 4:
            kw["nthread"] = 3
        _both_paths(dm, data, offs, want_fast=True, **kw)
    data = fuzz_ws.sized(lambda n: gen(n, 40), BIG)
    offs = fuzz_text.random_cuts(rng, data, 5)
    _both_paths(dm, data, offs, want_fast=True, delimiter=delim, value_type=VT[vt])
    assert _count_only_equals_full(dm, data, offs, delimiter=delim, value_type=VT[vt]) == 0


@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_gpu_ws_edges(dm, delim):
    """Class 3: runs across segment, tile and pre-halo boundaries, 62 and 64+
    blanks, chunk starts inside runs, a row over two tiles, CRLF, words, junk."""
    rng = np.random.default_rng(177 + DELIMS.index(delim))
    last = None
    for name, data, offs, fast, f32_only in fuzz_ws.edge_cases(delim):
        for vt in ("f32", "i32"):
            if offs is None:
                cuts = [fuzz_text.random_cuts(rng, data, 6, anywhere=True) for _ in range(4)]
            else:
                cuts = [[0, len(data)] if offs == "whole" else offs]
            for c in cuts:
                want = True if fast and not (f32_only and vt != "f32") else None
                _both_paths(dm, data, c, want_fast=want, delimiter=delim, value_type=VT[vt])
        if name == "row_over_two_tiles":
            last = data
    assert _count_only_equals_full(dm, last, [0, len(last)], delimiter=delim) == 0


@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_gpu_ws_violations(dm, delim):
    """Class 4: the reference's result whichever path runs, alone and after a
    tile of clean rows."""
    rng = np.random.default_rng(5)
    base = fuzz_ws.sized(lambda n: fuzz_ws.runs(rng, n, 20, delim), fuzz_ws.TILE + 100)
    for name, data, offs in fuzz_ws.violations(delim):
        for vt in ("f32", "i32", "i64"):
            _both_paths(dm, data, offs if offs is not None else [0, len(data)], delimiter=delim, value_type=VT[vt])
        big = base + data
        cuts = [0, len(base), len(big)] if offs is None else [0] + [len(base) + x for x in offs]
        _both_paths(dm, big, cuts, delimiter=delim)
    assert _count_only_equals_full(dm, big, cuts, delimiter=delim) in (0, 1)


@pytest.mark.parametrize("vt", ["i32", "i64"])
@pytest.mark.parametrize("delim", [",", "\t"], ids=["comma", "tab"])
def test_gpu_int_label_column(dm, delim, vt):
    """Class 5: integer DTypes with a label column on the single pass; an
    empty label field and the fatal one-field row go to the exact kernels."""
    rng = np.random.default_rng(400 + VT[vt] + (10 if delim == "\t" else 0))
    ncols = 7
    for it, lc in enumerate((0, 1, ncols - 1, 0, 1, ncols - 1)):
        data = fuzz_text.labeled_csv(rng, int(rng.integers(1, 41)), ncols, lc, delim)
        kw = {"delimiter": delim, "value_type": VT[vt], "label_column": lc, "index_bits": 64 if it == 2 else 32}
        if it >= 3:
            kw["weight_column"] = (2, 0, 3)[it - 3]  # an ordinary column for integer DTypes
        if it == 5:
            kw["nthread"] = 3
        h = _both_paths(dm, data, fuzz_text.random_cuts(rng, data, 4), want_fast=True, **kw)
        assert h["label"].dtype == (np.int32 if vt == "i32" else np.int64) and len(h["label"]) == len(h["offset"]) - 1
    data = fuzz_ws.sized(lambda n: fuzz_text.labeled_csv(rng, n, 12, 0, delim), BIG)
    offs = fuzz_text.random_cuts(rng, data, 5)
    _both_paths(dm, data, offs, want_fast=True, delimiter=delim, value_type=VT[vt], label_column=0)
    assert _count_only_equals_full(dm, data, offs, delimiter=delim, value_type=VT[vt], label_column=0) == 0
    for kind, lc in (("empty", 0), ("empty", 2), ("one_field", 0)):
        data = fuzz_ws.int_label_defect(rng, 12, ncols, lc, kind, delim)
        o = po.parse_chunks(data, [0, len(data)], fmt=po.CSV, delimiter=delim, value_kind=VT[vt], label_column=lc)
        assert (o["status"] != 0) == (kind == "one_field"), o["msg"]  # "Delimiter not found" must be raised
        _both_paths(dm, data, [0, len(data)], want_fast=False, delimiter=delim, value_type=VT[vt], label_column=lc)


def test_gpu_float_label_weight_columns_tab(dm):
    """Class 6: the label / weight kernel with '\\t': clean inputs stay on the
    single pass, a doubled delimiter declines and matches."""
    rng = np.random.default_rng(166)
    for it, (lc, wc) in enumerate(((0, -1), (2, -1), (-1, 1), (0, 2), (3, 1), (1, 4))):
        ncols = max(lc, wc) + 2 + int(rng.integers(0, 6))
        big = it == 3
        data = fuzz_text.labeled_csv(rng, 40, ncols, lc, "\t", weight_col=wc) if not big else fuzz_ws.sized(
            lambda n: fuzz_text.labeled_csv(rng, n, ncols, lc, "\t", weight_col=wc), BIG)
        kw = {"delimiter": "\t", "label_column": lc, "weight_column": wc}
        offs = fuzz_text.random_cuts(rng, data, 4)
        _both_paths(dm, data, offs, want_fast=True, **kw)
        if big:
            assert _count_only_equals_full(dm, data, offs, **kw) == 0
        else:
            _both_paths(dm, fuzz_ws.doubled(data, "\t", rng), [0, len(data) + 1], want_fast=False, **kw)
    for text in ("\t1\t2\t3\n", "1\t2\t3\t\n4\t5\t6\n", "1\t 2\t3\n"):
        _both_paths(dm, text.encode(), [0, len(text)], want_fast=False, delimiter="\t", label_column=1)


_MID = {}


def _mid_text():
    if "t" not in _MID:
        _MID["t"] = synth.rows(synth.CSV, 4096, 64, seed=3)[0].tobytes()
    return _MID["t"]


@pytest.mark.parametrize("vt", ["f32", "i32", "i64"])
@pytest.mark.parametrize("delim", DELIMS, ids=["tab", "space"])
def test_gpu_ws_mid_size_fast_equals_exact(dm, delim, vt):
    """About 0.8 MB, some 50 tiles: the look-back carries the segmented column
    count over many tiles; single pass == exact kernels == oracle, bit for bit."""
    data = fuzz_ws.with_delim(_mid_text(), delim)
    assert len(data) > 40 * fuzz_ws.TILE
    offs = [0, data.index(b"\n", len(data) // 3) + 1, len(data)]
    hf = _oracle_vs_gpu(dm, data, offs, want_fast=True, delimiter=delim, value_type=VT[vt])
    he = _oracle_vs_gpu(dm, data, offs, want_fast=False, delimiter=delim, value_type=VT[vt], exact=True)
    for k in ("offset", "label", "weight", "index", "value", "chunk_table"):
        assert np.asarray(hf[k]).tobytes() == np.asarray(he[k]).tobytes(), k


# ------------------------------------------------------------ C++ Parser --


def test_api_tsv_directory(tmp_path):
    """Parser<uint32_t,float>::Create(uri + "?format=csv&delimiter=<tab>") over
    a two-file directory: the blocks equal the oracle's."""
    from test_host_api import _write, oracle_files, run_api
    files = [fuzz_ws.with_delim(synth.rows(synth.CSV, 300, 12, seed=s)[0].tobytes(), "\t") for s in (5, 6)]
    d, _ = _write(tmp_path / "tsv", files)
    h = run_api(tmp_path, d + "?format=csv&delimiter=\t", fmt="auto")
    o, _ = oracle_files(files, fmt=po.CSV, d=d, delimiter="\t")
    assert "error" not in h, h
    assert diff(h, o) == [] and len(h["offset"]) - 1 == 600
    assert h["blocks"].tolist() == o["blocks"]["rows"].tolist()


def test_api_int32_label_column(tmp_path):
    """Parser<uint32_t,int32_t> with label_column=0 on a ',' file."""
    from test_host_api import _write, oracle_files, run_api
    rng = np.random.default_rng(8)
    files = [fuzz_text.labeled_csv(rng, 500, 9, 0)]
    d, _ = _write(tmp_path / "ilab", files)
    h = run_api(tmp_path, d + "?format=csv&label_column=0", fmt="auto", dtype="i32")
    o, _ = oracle_files(files, fmt=po.CSV, d=d, value_kind=po.I32, label_column=0)
    assert "error" not in h, h
    assert diff(h, o) == [] and h["label"].dtype == np.int32 and len(h["label"]) == 500
    assert h["blocks"].tolist() == o["blocks"]["rows"].tolist()
