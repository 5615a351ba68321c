"""GPU parity for the float label / weight kernel of the single-pass CSV family
(csv_fast.h tile<MODE, true, 0, false>; csv.hip csv_fast_tile_sp) on header
rows, text, missing values, blanks and BOMs.

Through the C ABI (dmlc_amd.parse_bytes) and through the C++ Parser.  Every
comparison is bit-exact on offset / label / weight / index / value against the
oracle or the reference's recorded arrays; the classes of tests/fuzz_csv_sp.py
that are inside the single-pass grammar by construction must report
path == "fast" for every case, the violations path == "exact"."""
import numpy as np
import pytest

import fuzz_csv_sp as fz
import fuzz_text
from fuzz_ws import TILE
from golden_util import dec, diff, load_json
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

BIG = 3 * TILE + 321
FIXTURE = load_json("csv_sp_text.json")


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
    o = po.parse_chunks(data, offs, fmt=po.CSV, **{k: v for k, v in kw.items() if k != "exact"})
    h = gpu_parse(dm, data, offs, **kw)
    assert (o["status"] != 0) == h["failed"], (o["msg"], h["error"], data[:200], offs, kw)
    if o["status"] == 0:
        bad = diff(h, o)
        assert bad == [], (bad, data[:200], offs, kw)
    if want_fast is not None:
        assert (h["path"] == "fast") == want_fast, (h["path"], data[:200], offs, kw)
    return h


def _both_paths(dm, data, offs, want_fast=None, **kw):
    """The default path and FLAG_EXACT both equal the oracle, and each other's per-unit table."""
    h = _oracle_vs_gpu(dm, data, offs, want_fast=want_fast, **kw)
    he = _oracle_vs_gpu(dm, data, offs, want_fast=False, exact=True, **kw)
    if not h["failed"]:
        assert h["chunk_table"].tolist() == he["chunk_table"].tolist()
        for k in ("offset", "label", "weight", "index", "value"):
            assert np.asarray(h[k]).tobytes() == np.asarray(he[k]).tobytes(), k
    return h


def _count_then_fill_equals_full(dm, data, offs, **kw):
    """COUNT_ONLY, then FILL_ONLY into buffers of exactly those sizes, against
    one full call: the same totals and arrays.  Returns the full call's path
    (0 = single pass)."""
    import torch
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    p = dm.DeviceParser("csv", **kw)
    two = p.parse(text, cs)  # COUNT_ONLY, then FILL_ONLY
    counts = [int(x) for x in two["counts"][:8]]
    assert two["error"] == 0 and two["result_counts"] == counts
    out = p.alloc(counts)
    res = torch.zeros(16, dtype=torch.int64, device="cuda")
    p.parse_into(text, cs, out, res)
    r = res.cpu().numpy().view(np.uint64)
    assert int(r[8]) == 0 and [int(x) for x in r[:8]] == counts, (counts, r[:10])
    assert bool(two["path"]) == bool(r[9])
    n = {"offset": counts[0] + 1, "index": counts[1], "value": counts[2], "weight": counts[3], "label": counts[5]}
    for k, m in n.items():
        assert torch.equal(out[k][:m].view(torch.uint8), two[k][:m].view(torch.uint8)), k
    return int(r[9])


def test_gpu_reference_fixture(dm):
    """What the genuine reference recorded for the table, the small edge cases
    and the violations; the single pass wherever it must stand, the exact
    kernels for every violation."""
    for case in FIXTURE:
        prm = case["params"]
        h = gpu_parse(dm, case["data_latin1"].encode("latin-1"), case["offs"], delimiter=prm["delimiter"],
                      label_column=prm["label_column"], weight_column=prm["weight_column"])
        assert h["failed"] == bool(case["status"]), (case["name"], h["error"], case["msg"])
        if not case["status"]:
            exp = {k: dec(v) for k, v in case["expect"].items()}
            assert diff(h, exp) == [], (case["name"], diff(h, exp))
        if case["fast"]:
            assert h["path"] == "fast", case["name"]
        if case["exact"]:
            assert h["path"] == "exact", case["name"]


@pytest.mark.parametrize("form", fz.FORMS, ids=["l0", "l1", "llast", "l0w2", "l3w1"])
@pytest.mark.parametrize("cls", fz.CLASSES)
def test_gpu_classes_stay_single_pass(dm, cls, form):
    """Headers, text and missing values, blanks, BOMs: always the single pass,
    equal to the oracle and to FLAG_EXACT; one input of three tiles and a bit,
    on which COUNT_ONLY then FILL_ONLY equals one full call."""
    rng = np.random.default_rng(5000 + 10 * fz.CLASSES.index(cls) + fz.FORMS.index(form))
    for it in range(6):
        data, lc, wc = fz.gen(rng, cls, int(rng.integers(1, 41)), form)
        kw = {"label_column": lc, "weight_column": wc, "index_bits": 64 if it % 3 == 1 else 32}
        if it == 4:
            kw["nthread"] = 3
        # (BOMs: one input with a chunk cut at every later row-start BOM)
        cuts = fz.bom_cuts(data) if cls == "boms" and it == 5 else fuzz_text.random_cuts(rng, data, 4)
        _both_paths(dm, data, cuts, want_fast=True, **kw)
    data, lc, wc = fz.sized(rng, cls, form, BIG)
    offs = fuzz_text.random_cuts(rng, data, 5)
    _both_paths(dm, data, offs, want_fast=True, label_column=lc, weight_column=wc)
    assert _count_then_fill_equals_full(dm, data, offs, label_column=lc, weight_column=wc) == 0


def test_gpu_label0_text_row_longer_than_a_tile(dm):
    rng = np.random.default_rng(12)
    words = ["NA", "", "?", "abc", "1.5", "x", "nan", ""]
    rows = []
    for n in (5000, 12, 9000, 3):
        rows.append(",".join(words[int(x)] for x in rng.integers(0, len(words), size=n)) + ",1")
    data = ("\n".join(rows) + "\n").encode()
    assert len(data) > 2 * TILE
    _both_paths(dm, data, [0, len(data)], want_fast=True, label_column=0)


def test_gpu_edges(dm):
    """Tokenless special fields in a carried-in row, label fields cut by
    segment and tile boundaries, a header longer than a tile, CRLF, and a BOM
    before 61..130 blanks around a segment boundary (labelled, plain, tab)."""
    for name, data, lc, wc, delim, fast in fz.edge_cases():
        _oracle_vs_gpu(dm, data, [0, len(data)], want_fast=fast, label_column=lc, weight_column=wc, delimiter=delim)


def test_gpu_violations(dm):
    """A NaN weight (one row, every row), a short row, an empty last-column
    label, a one-field row under label_column=0: the exact kernels and the
    reference's result or error, alone and behind a tile of text rows; the
    size query and the fill agree with one full call."""
    rng = np.random.default_rng(5)
    for name, text, lc, wc in fz.violations():
        data = text.encode("latin-1")
        _both_paths(dm, data, [0, len(data)], want_fast=False, label_column=lc, weight_column=wc)
        ncols = text.split("\n")[0].count(",") + 1
        base = fz.sized(rng, "text", (lc, wc), TILE + 100, ncols)[0]
        big = base + data
        cuts = [0, len(base), len(big)]
        h = _both_paths(dm, big, cuts, want_fast=False, label_column=lc, weight_column=wc)
        if not h["failed"]:
            assert _count_then_fill_equals_full(dm, big, cuts, label_column=lc, weight_column=wc) == 1, name


def _behind_header(text, width):
    header = (",".join("feature_%d" % j for j in range(width)) + "\n").encode()
    return header + text.tobytes()


@pytest.mark.parametrize("kind", ["CSV", "CSV_SP", "CSV_NAN"])
def test_gpu_header_6000_x256_label_column(dm, kind):
    """The flagship shape cut to 6000 rows behind a header row, label_column 0
    and 5: the single pass, 6000 labels plus the header's 0."""
    text, _ = synth.rows(getattr(synth, kind), 6000, 256, seed=17)
    data = _behind_header(text, 256)
    offs = dm.text_chunk_starts(np.frombuffer(data, np.uint8), 1 << 20).tolist()
    for lc in (0, 5):
        h = _oracle_vs_gpu(dm, data, offs, want_fast=True, label_column=lc)
        assert len(h["label"]) == 6001 and h["label"][0] == 0


def test_api_header_label_column(tmp_path):
    """Parser<uint32_t,float> over a file with a header row, "?format=csv&label_column=0"."""
    from test_host_api import _write, oracle_files, run_api
    rng = np.random.default_rng(8)
    files = [b"label,f0,f1,name,inf_x,w,x,y,z\n" + fuzz_text.labeled_csv(rng, 500, 9, 0)]
    d, _ = _write(tmp_path / "hlab", files)
    h = run_api(tmp_path, d + "?format=csv&label_column=0", fmt="auto")
    o, _ = oracle_files(files, fmt=po.CSV, d=d, label_column=0)
    assert "error" not in h, h
    assert diff(h, o) == [] and len(h["label"]) == 501 and h["label"][0] == 0
    assert h["blocks"].tolist() == o["blocks"]["rows"].tolist()
