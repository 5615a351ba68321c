"""TEST INFRASTRUCTURE ONLY -- the one-call parse pipeline against the oracle.

dmlc_amd.parse_bytes drives dmlc_amd_parse as COUNT_ONLY, an exact-size
allocation, then FILL_ONLY.  The host engine (host/hip_engine.h) and bench.py
make ONE call with flags = 0 into outputs whose capacities are guesses; this
module drives that form:

parse_full()      one parse_into call, no count phase before it on that
                  parser, into outputs of `cap + GUARD` elements pre-filled
                  with a sentinel; every element at or past the capacity must
                  still be the sentinel afterwards.
full_vs_oracle()  parse_full compared with the oracle: failure status, exact
                  counts, every array bit for bit, and the unit table against
                  the one the split pipeline returns.
*_cases()         the inputs of tests/test_gpu_full_call.py, built from the
                  generators of fuzz_text / fuzz_ws, each with the path it must
                  take where that is known by construction ("stay" on the
                  single pass, "hand" over to the exact kernels inside the
                  call); the same lists run through the CPU emulator.
"""
import ctypes
import re

import numpy as np

import fuzz_text
import fuzz_ws
from golden_util import diff
from oracle import pyoracle as po
from tools import synth

FMT_NAME = {po.LIBSVM: "libsvm", po.CSV: "csv", po.LIBFM: "libfm"}
ARRAYS = ("offset", "label", "weight", "qid", "field", "index", "value")
GUARD = 64        # elements behind every output's capacity
SENT_BYTE = 0x5A  # every guard byte (0x5A5A5A5A as int32 / float bits, as test_gpu_umin_fix_stays_inside_capacity)
ROWS, INDEX, VALUE, WEIGHT, QID, LABEL, FIELD = range(7)
FLAG_EXACT, FLAG_MAX_INDEX = 4, 8


# --------------------------------------------------------------- oracle --
def oracle_kw(params):
    """The oracle's keywords for a dmlc_amd parameter block."""
    return dict(index_bits=int(params.index_bits), value_kind=int(params.value_type),
                indexing_mode=int(params.indexing_mode), label_column=int(params.label_column),
                weight_column=int(params.weight_column), delimiter=int(params.delimiter),
                nthread=max(int(params.nthread), 1))


def oracle_counts(o):
    """dmlc_amd_result.count[:7] an oracle result stands for (dmlc_amd.h slots)."""
    return [len(o["offset"]) - 1, len(o["index"]), len(o["value"]), len(o["weight"]), len(o["qid"]),
            len(o["label"]), len(o["field"])]


def make_parser(dm, fmt, kw):
    kw = dict(kw)
    if kw.pop("exact", False):
        kw["flags"] = kw.get("flags", 0) | FLAG_EXACT
    return dm.DeviceParser(FMT_NAME.get(fmt, fmt), **kw)


def _fmt_of(params):
    return (po.LIBSVM, po.CSV, po.LIBFM)[int(params.format)]


def split_kw(params):
    """parse_bytes keywords for the same parameters (the split pipeline)."""
    return dict(index_bits=int(params.index_bits), value_type=int(params.value_type),
                indexing_mode=int(params.indexing_mode), label_column=int(params.label_column),
                weight_column=int(params.weight_column), delimiter=int(params.delimiter),
                tile_bytes=int(params.tile_bytes), nthread=int(params.nthread),
                flags=int(params.flags) & FLAG_EXACT)


# -------------------------------------------------------------- outputs --
def _dtypes(params):
    it = np.uint32 if params.index_bits == 32 else np.uint64
    vt = {0: np.float32, 1: np.int32, 2: np.int64}[int(params.value_type) if params.format == 1 else 0]
    return {"offset": np.uint64, "label": vt, "weight": np.float32, "qid": np.uint64, "field": it, "index": it,
            "value": vt}


def array_caps(params, caps):
    """Elements the call may write per output array: cap[ROWS] + 1 offsets;
    labels go by cap[LABEL] for CSV and by cap[ROWS] otherwise (dmlc_amd.h:
    LABEL is a CSV slot, "cap[ROWS] counts labels")."""
    lab = caps[LABEL] if params.format == 1 else caps[ROWS]
    return {"offset": caps[ROWS] + 1, "label": lab, "weight": caps[WEIGHT], "qid": caps[QID],
            "field": caps[FIELD], "index": caps[INDEX], "value": caps[VALUE]}


def new_outputs(params, elems):
    """One output set: byte tensors of (elems[k] + GUARD) elements each."""
    import torch
    dt = _dtypes(params)
    return {k: torch.empty((int(elems[k]) + GUARD) * np.dtype(dt[k]).itemsize, dtype=torch.uint8, device="cuda")
            for k in ARRAYS}


def parse_full(dm, data, offs, fmt, caps=None, slack=0, parser=None, result=None, outputs=None, oracle=None, **kw):
    """ONE dmlc_amd_parse call (flags without COUNT_ONLY / FILL_ONLY) on
    `parser` (a new DeviceParser(fmt, **kw) when None; exact=True sets
    FLAG_EXACT) into sentinel-filled outputs.

    caps: the seven capacities (dmlc_amd.h slot order); by default the
    oracle's array lengths + slack, or len(data) + 2 in every slot when the
    oracle reports an error.  result: a device int64[16] block to reuse.
    outputs: a new_outputs() set to reuse (refilled with the sentinel).
    Returns a host dict like parse_bytes': offset ... value trimmed to
    min(count, capacity), counts, error, path (the raw word), chunk_table,
    units_per_chunk, caps, max_index.  Asserts the guard bands."""
    import torch
    raw = data.encode("latin-1") if isinstance(data, str) else bytes(data)
    offs = [int(x) for x in offs] if offs is not None else ([0, len(raw)] if raw else [0])
    if parser is None:
        parser = make_parser(dm, fmt, kw)
    else:
        assert not kw, "a reused parser keeps its parameters"
    prm = parser.params
    if caps is None:
        o = oracle if oracle is not None else po.parse_chunks(raw, offs, fmt=_fmt_of(prm), **oracle_kw(prm))
        caps = [len(raw) + 2] * 7 if o["status"] else [c + slack for c in oracle_counts(o)]
    caps = [int(c) for c in caps[:7]]
    acap = array_caps(prm, caps)
    dt = _dtypes(prm)
    if outputs is None:
        outputs = new_outputs(prm, acap)
    for k in ARRAYS:
        assert outputs[k].numel() >= (acap[k] + GUARD) * np.dtype(dt[k]).itemsize, k
        outputs[k].fill_(SENT_BYTE)
    text = torch.frombuffer(bytearray(raw), dtype=torch.uint8).cuda() if raw else \
        torch.empty(0, dtype=torch.uint8, device="cuda")
    cs = torch.tensor(np.asarray(offs, dtype=np.int64), device="cuda")
    nchunks = len(offs) - 1
    upc = dm.units_per_chunk(prm)
    nrows = max(nchunks * upc, 1)
    tab = torch.full(((nrows * 8 + GUARD) * 8,), SENT_BYTE, dtype=torch.uint8, device="cuda")
    tab[:nrows * 64].zero_()  # as DeviceParser.parse hands it over
    res = result if result is not None else torch.zeros(16, dtype=torch.int64, device="cuda")
    csr = dm.Csr()
    for k in ARRAYS:
        setattr(csr, k, outputs[k].data_ptr())
    for i, c in enumerate(caps):
        csr.cap[i] = c
    parser.parse_into(text, cs, {"_csr": csr}, res, chunk_table=tab.view(torch.int64) if nchunks > 0 else None)
    torch.cuda.synchronize()
    r = res.cpu().numpy().view(np.uint64)
    counts = [int(x) for x in r[:8]]
    cnt = array_caps(prm, counts)
    h, touched = {}, []
    for k in ARRAYS:
        b = outputs[k].cpu().numpy()
        isz = np.dtype(dt[k]).itemsize
        if not (b[acap[k] * isz:] == SENT_BYTE).all():
            touched.append(k)
        h[k] = b[:min(cnt[k], acap[k]) * isz].view(dt[k])
    tb = tab.cpu().numpy()
    if not (tb[nrows * 64:] == SENT_BYTE).all():
        touched.append("chunk_table")
    assert touched == [], ("written at or past the capacity", touched, caps, counts)
    h["chunk_table"] = tb[:nrows * 64].view(np.uint64).reshape(-1, 8)
    h.update(counts=counts, error=int(r[8]), path=int(r[9]), max_index=int(r[10]), max_field=int(r[11]),
             units_per_chunk=upc, caps=caps)
    return h


def split_table(dm, data, offs, params):
    """The unit table of the split pipeline (count, allocate, fill) for the same input and parameters."""
    return dm.parse_bytes(data, offs, fmt=FMT_NAME[_fmt_of(params)], **split_kw(params))["chunk_table"]


def full_vs_oracle(dm, data, offs, fmt, split=None, oracle=None, parser=None, **kw):
    """parse_full against the oracle; returns its dict (h["oracle"]: the oracle's)."""
    raw = data.encode("latin-1") if isinstance(data, str) else bytes(data)
    offs = [int(x) for x in offs] if offs is not None else ([0, len(raw)] if raw else [0])
    pkeys = ("caps", "slack", "result", "outputs")
    pf = {k: kw.pop(k) for k in pkeys if k in kw}
    if parser is None:
        parser = make_parser(dm, fmt, kw)
    else:
        assert not kw, "a reused parser keeps its parameters"
    prm = parser.params
    name = FMT_NAME[_fmt_of(prm)]
    o = oracle if oracle is not None else po.parse_chunks(raw, offs, fmt=_fmt_of(prm), **oracle_kw(prm))
    h = parse_full(dm, raw, offs, fmt, parser=parser, oracle=o, **pf)
    nunits = (len(offs) - 1) * h["units_per_chunk"]
    failed = bool(h["error"]) or (nunits > 0 and dm.chunk_check(h, name, nunits, h["counts"]) >= 0)
    assert (o["status"] != 0) == failed, (o["msg"], h["error"], h["path"], raw[:200], offs)
    if o["status"] == 0:
        assert h["counts"][:7] == oracle_counts(o), (h["counts"], oracle_counts(o), h["path"])
        bad = diff(h, o)
        assert bad == [], (bad, h["path"], h["caps"], offs)
        s = split if split is not None else split_table(dm, raw, offs, prm)
        assert h["chunk_table"].tolist() == np.asarray(s).tolist(), ("unit table", h["path"], offs)
        if prm.flags & FLAG_MAX_INDEX:  # as the host engine calls it
            for key, got in (("index", h["max_index"]), ("field", h["max_field"])):
                if len(o[key]):
                    assert got == int(np.asarray(o[key]).max()), (key, got)
    h["oracle"] = o
    return h


def under_sized(dm, data, offs, fmt, caps, parser, result, oracle):
    """A call whose capacities are too small: ERR_CAPACITY, exact counts,
    nothing past a capacity; then the engine's retry (hip_engine.h: one more
    call on the same parser and result block with the failed call's counts as
    capacities), which must equal the oracle."""
    h = parse_full(dm, data, offs, fmt, caps=caps, parser=parser, result=result)
    assert dm.error_code(h["error"]) == dm.ERR_CAPACITY, (h["error"], caps, h["counts"])
    assert h["counts"][:7] == oracle_counts(oracle), (h["counts"], oracle_counts(oracle), caps)
    return full_vs_oracle(dm, data, offs, fmt, parser=parser, result=result, oracle=oracle, caps=h["counts"][:7])


# ---------------------------------------------------------------- inputs --
def lf(data):
    """'\\n' line ends only (a placed line must not land inside a "\\r\\n")."""
    return data.replace(b"\r\n", b"\n").replace(b"\r", b"\n")


def valued_lines(data, fmt, **okw):
    """The generated text without the lines that, parsed on their own, raise
    in the reference or hold a feature without a value: one such line among
    valued ones fails the reference's RowBlock CHECK (row_block.h:178) for its
    whole chunk, and then only the failure could be compared, not the arrays.
    Each line is parsed behind a '\\n', as it stands in the middle of a text:
    there a "# ..." line is no comment and its digits are a row
    (fuzz_text.comment_libsvm, line_comments), so a header that a block of
    grown() brings into the middle of the text is judged as the reference
    will read it; at a chunk start, where it is a comment, it is harmless.
    A filter over the generators' output, decided by the oracle -- no grammar
    of its own."""
    L = po.oracle_lib()
    prm = po.params(fmt=fmt, **okw)
    parts = re.split(b"(\r\n|\r|\n)", data)
    out = []
    for i in range(0, len(parts), 2):
        line, sep = parts[i], parts[i + 1] if i + 1 < len(parts) else b""
        if line.strip():
            buf = ctypes.create_string_buffer(b"\n" + line + b"\n", len(line) + 3)
            c = po.Csr()
            L.dmo_csr_init(ctypes.byref(c), prm.value_kind)
            L.dmo_parse_block(ctypes.cast(buf, ctypes.c_void_p), len(line) + 2, ctypes.byref(prm), ctypes.byref(c))
            ok = c.status == 0 and c.n_index == c.n_value
            L.dmo_csr_free(ctypes.byref(c))
            if not ok:
                continue
        out.append(line + sep)
    return b"".join(out)


def place_violation(clean, line, tile_index, tile):
    """`clean` ('\\n'-ended lines) with `line` and an empty line after it
    spliced in at a line start inside single-pass tile `tile_index` (past its
    middle, or at the end of the text when the tile is the short last one).
    Returns (data, (a, b)): [a, b) is the empty line -- as a chunk of its own
    it is a unit without a line, whose table row no exact tile writes."""
    assert clean.endswith(b"\n") and len(clean) > tile_index * tile
    want = tile_index * tile + tile // 2
    k = clean.index(b"\n", want) + 1 if want < len(clean) - 1 else len(clean)
    ins = line + b"\n\n"
    assert tile_index * tile <= k and k + len(ins) <= (tile_index + 1) * tile, (k, tile_index)
    data = clean[:k] + ins + clean[k:]
    a = k + len(line) + 1
    return data, (a, a + 1)


def empty_line_cut(data, lo, hi):
    """(a, a + 1) of the first empty line inside [lo, hi), or (): as a chunk
    of its own, a unit without a line in a tile the single pass has written
    before a later tile hands over."""
    k = data.find(b"\n\n", lo, hi)
    return (k + 1, k + 2) if k >= 0 else ()


def with_cuts(offs, extra):
    return sorted(set(offs) | set(extra))


def _case(name, data, offs, expect=None, parsed=False, **kw):
    """expect: "stay" / "hand" / None; parsed: the oracle must parse it (so the arrays are compared)."""
    return {"name": name, "data": data, "offs": offs, "expect": expect if data else None, "parsed": parsed,
            "kw": kw}  # (empty input: no single pass)


def _svm_kw(i):
    kw = {"indexing_mode": (i // 2) % 3 - 1, "nthread": 1 + i % 3}
    if i % 4 == 1:
        kw["index_bits"] = 64
    if i % 2:
        kw["flags"] = FLAG_MAX_INDEX
    return kw


def _multi(rng, tile):
    """A multi-tile size: 4-12 tiles, the small ones more often (the text generators are slow)."""
    return int(rng.choice([4, 4, 5, 5, 6, 7, 9, 11])) * tile + int(rng.integers(100, tile))


def grown(gen, nbytes):
    """About nbytes of gen(nlines) text: blocks of 96 lines appended until
    there is enough (fuzz_ws.sized regenerates everything at twice the lines),
    cut at a line end."""
    blocks, n = [], 0
    while n < nbytes + 200:
        d = gen(96)
        if d[-1:] not in (b"\n", b"\r"):
            d += b"\n"
        blocks.append(d)
        n += len(d)
    data = b"".join(blocks)
    return data[:data.index(b"\n", nbytes - 40) + 1]


def valued(gen, fmt, on=True):
    """gen(nlines) passed through valued_lines (on=False: as generated)."""
    return (lambda n: valued_lines(gen(n), fmt)) if on else gen


def svm_cases(tile):
    """libsvm inputs of the 2a fuzz: about half single-tile, half of 4-12
    tiles.  Each class of the tables below is drawn filtered (valued_lines: the
    oracle parses it, the arrays are compared) and as generated (mostly the
    reference's RowBlock CHECK failure, which is compared as such)."""
    rng = np.random.default_rng(20250)
    ft = fuzz_text
    cases = []
    # (class, generator(nlines, maxfeat), path of a clean input)
    small = [
        ("uniform", lambda n, mf: ft.uniform_libsvm(rng, n, mf), "stay"),
        ("uniform_violate", lambda n, mf: ft.uniform_libsvm(rng, n, mf, violate=True), None),
        ("qid", lambda n, mf: ft.qid_libsvm(rng, n, 16), "stay"),
        ("qid_violate", lambda n, mf: ft.qid_libsvm(rng, n, 16, violate=True), None),
        ("qid_mixed", lambda n, mf: ft.qid_libsvm(rng, n, 16, mixed=True), None),
        ("comment", lambda n, mf: ft.comment_libsvm(rng, n, 16), "stay"),
        ("comment_long_violate", lambda n, mf: ft.comment_libsvm(rng, n, 16, long_frac=0.2, violate=True), None),
        ("dirty_rows", lambda n, mf: ft.dirty_rows_libsvm(rng, max(n, 4), 4 + mf, rate=0.5, runs=mf % 2 == 1), "stay"),
        ("dirty_lines", lambda n, mf: ft.dirty_libsvm(rng, 2000, rate=0.05, long_frac=0.5, eol=(b"\n", b"\r\n")[mf % 2]), None),
    ]
    i = 0
    for rep, filtered in enumerate((True, True, False)):  # single-tile: 1-40 lines
        for cls, gen, expect in small:
            anywhere = i % 5 == 4
            data = gen(int(rng.integers(1, 41)), int(rng.integers(0, 14 if filtered else 40)))
            if filtered:
                data = valued_lines(data, po.LIBSVM)
            offs = ft.random_cuts(rng, data, 6, anywhere=anywhere)
            cases.append(_case("small_%s_%d" % (cls, rep), data, offs, None if anywhere else expect,
                               filtered and not anywhere, **_svm_kw(i)))
            i += 1
    # (class, generator(nlines, maxfeat) for grown(), or generator(nbytes) when sized by bytes, path)
    multi = [
        ("uniform", lambda n, mf: ft.uniform_libsvm(rng, n, mf), "stay", False),
        ("uniform_violate", lambda n, mf: ft.uniform_libsvm(rng, n, mf, violate=True), None, False),
        ("qid", lambda n, mf: ft.qid_libsvm(rng, n, 40), "stay", False),
        ("qid_violate", lambda n, mf: ft.qid_libsvm(rng, n, 40, violate=True), None, False),
        ("qid_mixed", lambda n, mf: ft.qid_libsvm(rng, n, 40, mixed=True), None, False),
        ("comment_long", lambda n, mf: ft.comment_libsvm(rng, n, 12, long_frac=0.1), None, False),
        ("comment_qid", lambda n, mf: ft.comment_libsvm(rng, n, 12, long_frac=0.1, qid=True), None, False),
        ("dirty_lines", lambda nb, mf: ft.dirty_libsvm(rng, nb, rate=0.01, long_frac=0.3, near_tile_end=mf > 12), None, True),
        ("dirty_rows", lambda nb, mf: ft.dirty_rows_libsvm(rng, nb // (60 * 16 + 4), 60, rate=0.125, near_tile_end=True),
         "stay", True),
    ]
    for rep in range(2):  # multi-tile; the second draw of every other class stays as generated
        for k, (cls, gen, expect, by_bytes) in enumerate(multi):
            filtered = rep == 0 or k % 2 == 0
            anywhere = rep == 1 and cls == "uniform"
            nb, mf = _multi(rng, tile), 12 if filtered else 40
            g = valued(lambda n: gen(n, mf), po.LIBSVM, filtered)
            data = g(nb if filtered else nb * 3 // 5) if by_bytes else grown(g, nb)  # (dirty_libsvm overshoots)
            offs = ft.random_cuts(rng, data, 6, anywhere=anywhere)
            cases.append(_case("multi_%s_%d" % (cls, rep), data, offs, None if anywhere else expect,
                               filtered and not anywhere, **_svm_kw(i)))
            i += 1
    # clean text with ONE violating line in the first, a middle and the last tile
    placed = (("dangling", b"1 2:3 3:", lambda n: ft.uniform_libsvm(rng, n, 12)),
              ("x_on_qid", b"1 qid:5 x 2:3", lambda n: ft.qid_libsvm(rng, n, 40)),
              ("no_qid", b"1 2:3 4:5", lambda n: ft.qid_libsvm(rng, n, 40)))
    for j, (kind, line, gen) in enumerate(placed):
        base = lf(grown(valued(gen, po.LIBSVM), _multi(rng, tile)))
        nt = (len(base) + tile - 1) // tile
        for t in (0, nt // 2, nt - 1):
            data, empty = place_violation(base, line, t, tile)
            offs = with_cuts(ft.random_cuts(rng, data, 5), empty + empty_line_cut(data, 0, t * tile))
            kw = {"nthread": 1 + (j + t) % 3, "indexing_mode": (-1, 0, 1)[j]}
            cases.append(_case("placed_%s_t%d" % (kind, t), data, offs, "hand", True, **kw))
        cases.append(_case("base_%s" % kind, base, ft.random_cuts(rng, base, 5), "stay", True, indexing_mode=(-1, 0, 1)[j]))
    return cases


def blank_last(ncols):
    """A full row whose last field is one blank: the decoder would read on
    into the next line, so the single pass declines it (fuzz_text.blank_csv's
    violation); the reference parses it."""
    return b",".join([b"1", b"0.5", b"0.25"] + [b"1"] * (ncols - 4) + [b" "])


def csv_cases(tile):
    """CSV inputs of the 2a fuzz: every class of the table once single-tile
    (1-40 lines) and once at 4-12 tiles.  The generators leave nothing for
    valued_lines to do: only defect rows and the placed short row fail the
    reference's label / weight CHECK."""
    rng = np.random.default_rng(20251)
    ft = fuzz_text

    def labeled(lc, wc, defects=0.0):
        ncols = max(lc, wc) + 2 + int(rng.integers(0, 20))
        return (lambda n: ft.labeled_csv(rng, n, ncols, max(lc, 0), defects=defects, weight_col=wc),
                {"label_column": lc, "weight_column": wc})

    def ws(gen, d, vt):
        return lambda n: gen(rng, n, 30, d, ints=vt != 0), {"delimiter": d, "value_type": vt}

    # (class, (generator(nlines), parameters), path at 4-12 tiles, path single-tile) -- paths as the
    # existing GPU tests assert them per input (uniform_csv single-tile: only in aggregate there)
    table = [
        ("uniform_comma", (lambda n: ft.uniform_csv(rng, n, 40, ","), {}), "stay", None),
        ("uniform_semi", (lambda n: ft.uniform_csv(rng, n, 40, ";"), {"delimiter": ";"}), "stay", None),
        ("uniform_violate_bar", (lambda n: ft.uniform_csv(rng, n, 40, "|", violate=True), {"delimiter": "|"}), None, None),
        ("uniform_violate_comma", (lambda n: ft.uniform_csv(rng, n, 40, ",", violate=True), {}), None, None),
        ("junk_header", (lambda n: ft.junk_csv(rng, n, 16, ",", header=True), {}), "stay", "stay"),
        ("junk_nan_literal", (lambda n: ft.junk_csv(rng, n, 16, ",", header=False, violate=True), {}), "stay", "stay"),
        ("blank_f32", (lambda n: ft.blank_csv(rng, n, 25, ","), {"value_type": 0}), None, None),
        ("blank_i32_violate", (lambda n: ft.blank_csv(rng, n, 25, ",", ints=True, violate=True), {"value_type": 1}), None, None),
        ("blank_i64", (lambda n: ft.blank_csv(rng, n, 25, ",", ints=True), {"value_type": 2}), None, None),
        ("label_weight", labeled(0, 2), "stay", "stay"),
        ("weight_only", labeled(-1, 1), "stay", "stay"),
        ("label_after_weight", labeled(3, 1), "stay", "stay"),
        ("label_only", labeled(3, -1), "stay", "stay"),
        ("label_weight_defects", labeled(1, 4, defects=0.1), None, None),
        ("ws_clean_tab_f32", ws(fuzz_ws.clean, "\t", 0), "stay", "stay"),
        ("ws_clean_space_i32", ws(fuzz_ws.clean, " ", 1), "stay", "stay"),
        ("ws_runs_tab_i32", ws(fuzz_ws.runs, "\t", 1), "stay", "stay"),
        ("ws_runs_space_f32", ws(fuzz_ws.runs, " ", 0), "stay", "stay"),
    ]
    may_raise = {"junk_nan_literal"}  # stays on the single pass, but an unclosed "NaN(" is the reference's fatal error
    cases = []
    i = 0
    for size in ("small", "multi"):
        for cls, (gen, kw0), at_multi, at_small in table:
            kw = dict(kw0, nthread=1 + i % 3, **({"index_bits": 64} if i % 4 == 1 else {}))
            data = gen(int(rng.integers(1, 41))) if size == "small" else grown(gen, _multi(rng, tile))
            anywhere = size == "small" and i % 5 == 4 and not cls.startswith("ws_")  # (the ws classes are clean for cuts at line ends)
            offs = ft.random_cuts(rng, data, 6, anywhere=anywhere)
            expect = None if anywhere else (at_small if size == "small" else at_multi)
            cases.append(_case("%s_%s" % (size, cls), data, offs, expect, expect == "stay" and cls not in may_raise, **kw))
            i += 1
    placed = (("short_row", b"1,2", lambda n: ft.labeled_csv(rng, n, 9, 3), {"label_column": 3}, False),
              ("blank_last", blank_last(12), lambda n: ft.labeled_csv(rng, n, 12, 0, weight_col=2),
               {"label_column": 0, "weight_column": 2}, True))
    for j, (kind, line, gen, kw0, parsed) in enumerate(placed):
        base = lf(grown(gen, _multi(rng, tile)))
        nt = (len(base) + tile - 1) // tile
        for t in (0, nt // 2, nt - 1):
            data, empty = place_violation(base, line, t, tile)
            offs = with_cuts(ft.random_cuts(rng, data, 5), empty + empty_line_cut(data, 0, t * tile))
            cases.append(_case("placed_%s_t%d" % (kind, t), data, offs, "hand", parsed, nthread=1 + (j + t) % 3, **kw0))
        cases.append(_case("base_%s" % kind, base, ft.random_cuts(rng, base, 5), "stay", True, **kw0))
    return cases


def fm_cases(tile):
    """libfm inputs of the 2a fuzz: each class of the table six times
    single-tile and three times at 4-12 tiles; the draws named in `raw` stay
    as generated, the others pass valued_lines."""
    rng = np.random.default_rng(20252)
    ft = fuzz_text
    # (class, generator(nlines, width), path of a clean input)
    table = [
        ("uniform", lambda n, w: ft.uniform_libfm(rng, n, w), "stay"),
        ("uniform_violate", lambda n, w: ft.uniform_libfm(rng, n, w, violate=True), None),
        ("rows", lambda n, w: ft.libfm_rows(rng, n, 3 * w), "stay"),
        ("rows_weights", lambda n, w: ft.libfm_rows(rng, n, 3 * w, weights=True), "stay"),
    ]
    cases = []
    i = 0
    for size, reps, raw in (("small", 6, (3, 5)), ("multi", 3, (2,))):
        for rep in range(reps):
            for cls, gen, expect in table:
                kw = {"indexing_mode": i % 3 - 1, "nthread": 1 + (i // 3) % 3}
                if i % 4 == 1:
                    kw["index_bits"] = 64
                if i % 2:
                    kw["flags"] = FLAG_MAX_INDEX
                filtered = rep not in raw
                anywhere = i % 6 == 4 if size == "small" else i % 12 == 5
                g = valued(lambda n: gen(n, 10 if size == "small" else 8), po.LIBFM, filtered)
                data = g(int(rng.integers(1, 41))) if size == "small" else grown(g, _multi(rng, tile))
                offs = ft.random_cuts(rng, data, 6, anywhere=anywhere)
                parsed = not anywhere and (filtered or cls.startswith("rows"))  # (libfm_rows holds valued triples only)
                cases.append(_case("%s_%s_%d" % (size, cls, rep), data, offs, None if anywhere else expect, parsed, **kw))
                i += 1
    placed = (("chain", b"1 1:2:3:4", lambda n: ft.libfm_rows(rng, n, 30)),
              ("word", b"1 2:3:4 x", lambda n: ft.uniform_libfm(rng, n, 8)))
    for j, (kind, line, gen) in enumerate(placed):
        base = lf(grown(valued(gen, po.LIBFM), _multi(rng, tile)))
        nt = (len(base) + tile - 1) // tile
        for t in (0, nt // 2, nt - 1):
            data, empty = place_violation(base, line, t, tile)
            offs = with_cuts(ft.random_cuts(rng, data, 5), empty + empty_line_cut(data, 0, t * tile))
            kw = {"nthread": 1 + (j + t) % 3, "indexing_mode": (-1, 0)[j]}
            cases.append(_case("placed_%s_t%d" % (kind, t), data, offs, "hand", True, **kw))
        cases.append(_case("base_%s" % kind, base, ft.random_cuts(rng, base, 5), "stay", True, indexing_mode=(-1, 0)[j]))
    return cases


CASES = {po.LIBSVM: svm_cases, po.CSV: csv_cases, po.LIBFM: fm_cases}


def capacity_input(fmt, mode, tile):
    """(data, offs, kw) of the capacity contract: three tiles with every slot
    the format has in use; mode "stay" (clean), "hand" (one placed violating
    line in the middle tile) or "exact" (clean, FLAG_EXACT)."""
    rng = np.random.default_rng(777 + fmt)
    ft = fuzz_text
    nb = 2 * tile + tile // 2
    if fmt == po.LIBSVM:   # weights on a quarter of the rows, a qid on every row
        base, line, kw = lf(grown(valued(lambda n: ft.qid_libsvm(rng, n, 20), po.LIBSVM), nb)), b"1 2:3 4:5", {}
    elif fmt == po.CSV:
        base = grown(lambda n: ft.labeled_csv(rng, n, 10, 0, weight_col=2), nb)
        line, kw = blank_last(10), {"label_column": 0, "weight_column": 2}
    else:
        base, line, kw = grown(lambda n: ft.libfm_rows(rng, n, 12, weights=True), nb), b"1 1:2:3:4", {}
    assert 2 * tile < len(base) <= 3 * tile
    if mode == "hand":
        data, empty = place_violation(base, line, 1, tile)
        return data, with_cuts(ft.random_cuts(rng, data, 3), empty), kw
    if mode == "exact":
        kw["exact"] = True
    return base, ft.random_cuts(rng, base, 3), kw


def cluster_chunks(tile, max_cs):
    """The clustered many-chunks input of test_emu_fast_many_chunks: more
    unit starts inside tile 2 than svm_fast_tile takes (kMaxCs), which the
    lean kernel (63 per wave) keeps on the single pass."""
    rng = np.random.default_rng(91)
    text, _ = synth.rows(synth.LIBSVM, 2500, 12, seed=3)
    data = text.tobytes()
    a = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(a == 10) + 1
    nl = nl[nl < len(data)]
    mid = nl[(nl > 2 * tile) & (nl < 3 * tile)]
    assert len(data) > 3 * tile and len(mid) > max_cs
    cuts = set(rng.choice(nl, size=300, replace=False).tolist()) | set(mid.tolist())
    return data, [0] + sorted(cuts) + [len(data)]


def lean_cases(tile):
    """libsvm full calls of the lean-kernel child (tests/lean_child.py)."""
    rng = np.random.default_rng(20253)
    ft = fuzz_text
    cases = []
    for i in range(3):
        data = grown(valued(lambda n: ft.uniform_libsvm(rng, n, 12), po.LIBSVM, i != 0), _multi(rng, tile))
        cases.append(_case("uniform%d" % i, data, ft.random_cuts(rng, data, 6), "stay",
                           **({"index_bits": 64} if i == 1 else {"nthread": 2} if i == 2 else {})))
    data = grown(valued(lambda n: ft.uniform_libsvm(rng, n, 12, violate=True), po.LIBSVM), _multi(rng, tile))
    cases.append(_case("violate", data, ft.random_cuts(rng, data, 6)))
    base = lf(grown(valued(lambda n: ft.uniform_libsvm(rng, n, 12), po.LIBSVM), _multi(rng, tile)))
    nt = (len(base) + tile - 1) // tile
    for t in (0, nt // 2, nt - 1):
        data, empty = place_violation(base, b"1 2:3 3:", t, tile)
        cases.append(_case("placed_t%d" % t, data, with_cuts(ft.random_cuts(rng, data, 5), empty), "hand",
                           nthread=1 + t % 2))
    for i in range(2):
        data = grown(valued(lambda n: ft.qid_libsvm(rng, n, 40, mixed=i == 1), po.LIBSVM), _multi(rng, tile))
        cases.append(_case("qid%d" % i, data, ft.random_cuts(rng, data, 6)))
    data = grown(valued(lambda n: ft.comment_libsvm(rng, n, 12, long_frac=0.1), po.LIBSVM), _multi(rng, tile))
    cases.append(_case("comment", data, ft.random_cuts(rng, data, 6)))
    for i, style in enumerate(("pairs", "weights", "labels", "mixed")):
        data = ft.dense_libsvm(rng, (3 + i) * tile + int(rng.integers(0, 999)), style)
        cases.append(_case("dense_" + style, data, ft.random_cuts(rng, data, 6), "stay",
                           **({"index_bits": 64} if i % 2 else {})))
    text, _ = synth.rows(synth.LIBSVM, 40, 2048, seed=4)
    data = text.tobytes()
    cases.append(_case("wide_rows", data, ft.random_cuts(rng, data, 6), "stay"))
    data = grown(valued(lambda n: ft.uniform_libsvm(rng, n, 12), po.LIBSVM), _multi(rng, tile))
    cases.append(_case("auto_index", data, ft.random_cuts(rng, data, 6), "stay", indexing_mode=-1))
    for c in cases:  # all but the first (as generated) are parsed by the oracle: arrays compared
        c["parsed"] = c["name"] != "uniform0"
    return cases
