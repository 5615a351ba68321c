"""TEST INFRASTRUCTURE ONLY -- the inputs of the captured-graph tests
(tests/test_gpu_graph.py, run by tests/graph_child.py) and their CPU checks
(tests/test_graph_cases.py).

A captured graph freezes the host arguments of every call: the byte count, the
number of chunks, every pointer and every capacity.  What may change between
two replays is device data only.  So the inputs come in REPLAY FAMILIES: lists
of members (name, bytes, chunk_offsets, expectation) that all have the same
byte count and the same number of chunks:

    A   clean text                                        "stay"  (single pass)
    B   clean text, fewer and longer rows, other cuts      "stay"
    C   A's lines with one violating line in the middle tile  "hand"  (exact kernels)
    D   A's lines with one line the reference raises on    "error" (code, byte position)
    E   clean text of the shortest runs: more entries than the captured capacities  "capacity"

The captured capacities are the slot-wise maximum of the oracle's counts over
A, B and C plus SLACK.  Every member is three single-pass tiles plus REM bytes.
The text comes from the generators of fuzz_text (and full_call's valued()
filter), cut to the byte with the padding of test_gpu_prologue.pad_line: blanks
before a newline, or extra "<delimiter>0" fields for CSV.

chain_family() is one more family, CSV with label_column=0 and 257 feature
columns, sized from the post-parse calls' geometries, with two id lists for
the gather; chain_expect() runs the numpy models over the oracle's CSR for the
six-call chain parse -> gather_rows -> make_cuts -> to_bins, to_dense, to_csc.
"""
import numpy as np

import bins_model as bm
import csc_model as cm
import cuts_model as qm
import dense_model as dmod
import full_call as fc
import fuzz_text as ft
import gather_model as gm
from oracle import pyoracle as po

REM = 1237    # bytes past the third tile
SLACK = 8     # elements past the largest count of A, B and C in every captured capacity
U32, U64 = np.uint32, np.uint64
ERR_NEG_INDEX, ERR_CSV_DELIM, ERR_CAPACITY = 1, 3, 16
ORDER = ("A", "B", "C", "A", "D", "A", "E", "A")  # the replay order of every parse graph


# ------------------------------------------------------------ sizing --
def split_lines(data):
    """The '\\n'-ended lines of a text (full_call.lf first: no '\\r')."""
    data = fc.lf(data)
    if not data.endswith(b"\n"):
        data += b"\n"
    return [x + b"\n" for x in data.split(b"\n")[:-1]]


def pad(line, k, delim=None):
    """`line` made k bytes longer inside the single-pass grammar, as
    test_gpu_prologue.pad_line: blanks before the newline (delim None), or
    extra "<delim>0" / "<delim>00" fields (CSV; k >= 2)."""
    if k == 0:
        return line
    if delim is None:
        return line[:-1] + b" " * k + b"\n"
    assert k >= 2
    return line[:-1] + (delim + b"0") * ((k - 3) // 2 if k % 2 else k // 2) + ((delim + b"00") if k % 2 else b"") + b"\n"


def fit(lines, nbytes, delim=None, per_line=24, can_pad=None):
    """The longest prefix of `lines` that fits nbytes, padded to exactly
    nbytes: at most per_line bytes on each of its last lines (those can_pad
    accepts; never an empty line)."""
    least = 1 if delim is None else 2
    out, n = [], 0
    for x in lines:
        if n + len(x) > nbytes:
            break
        out.append(x)
        n += len(x)
    else:
        raise AssertionError("too few lines for %d bytes" % nbytes)
    k = nbytes - n
    while 0 < k < least:
        k += len(out.pop())
    i = len(out) - 1
    while k:
        assert i >= 0
        if len(out[i]) > 1 and (can_pad is None or can_pad(out[i])):
            step = min(k, per_line)
            if 0 < k - step < least:
                step -= least
            out[i] = pad(out[i], step, delim)
            k -= step
        i -= 1
    assert sum(len(x) for x in out) == nbytes
    return out


def with_line(lines, line, at):
    """`lines` with `line` put in at the first line start at or past byte `at`; -> (lines, its position)."""
    n = 0
    for i, x in enumerate(lines):
        if n >= at:
            return lines[:i] + [line + b"\n"] + lines[i:], n
        n += len(x)
    raise AssertionError("no line start at or past %d" % at)


def cuts_near(lines, targets):
    """Chunk offsets: 0, the first line start at or past each target, the end."""
    starts = np.concatenate([[0], np.cumsum([len(x) for x in lines])])
    c = [int(starts[int(np.searchsorted(starts, t))]) for t in targets]
    offs = [0] + c + [int(starts[-1])]
    assert all(a < b for a, b in zip(offs, offs[1:])), offs
    return offs


# ----------------------------------------------------------- families --
def _short_csv(rng, nbytes, ncols, delim):
    """Rows of one-digit fields (label first): the most entries a byte count holds."""
    out, n = [], 0
    while n < nbytes:
        line = delim.join(str(int(v)) for v in rng.integers(0, 10, size=ncols))
        out.append(line)
        n += len(line) + 1
    return ("\n".join(out) + "\n").encode()


def _int_csv(rng, nlines, ncols, delim):
    """Rows of ncols non-empty integer fields, a 0 / 1 label first."""
    out = []
    for _ in range(nlines):
        f = [str(int(rng.integers(0, 2)))] + [str(int(v)) for v in rng.integers(-10 ** 6, 10 ** 6, size=ncols - 1)]
        out.append(delim.join(f))
    return ("\n".join(out) + "\n").encode()


def _specs():
    """name -> (oracle format, parser keywords shared by the family's
    configurations, CSV delimiter or None, nchunks, line sources)."""
    V = fc.valued
    return {
        "libsvm": dict(
            fmt=po.LIBSVM, kw={}, delim=None, nchunks=3, seed=5100,
            a=lambda rng: V(lambda n: ft.uniform_libsvm(rng, n, 12), po.LIBSVM),
            b=lambda rng: V(lambda n: ft.uniform_libsvm(rng, n, 60), po.LIBSVM),
            e=lambda rng, nb: ft.dense_libsvm(rng, nb, "pairs"),
            violate=b"1 2:3 3:", error=(b"1 -3:1", 2, ERR_NEG_INDEX)),
        "csv": dict(
            fmt=po.CSV, kw={"label_column": 0, "weight_column": 2}, delim=b",", nchunks=4, seed=5200,
            a=lambda rng: lambda n: ft.labeled_csv(rng, n, 10, 0, weight_col=2),
            b=lambda rng: lambda n: ft.labeled_csv(rng, n, 30, 0, weight_col=2),
            e=lambda rng, nb: _short_csv(rng, nb, 12, ","),
            violate=fc.blank_last(10), error=(b"5", 1, ERR_CSV_DELIM)),
        "libfm": dict(
            fmt=po.LIBFM, kw={}, delim=None, nchunks=3, seed=5300,
            a=lambda rng: V(lambda n: ft.uniform_libfm(rng, n, 8), po.LIBFM),
            b=lambda rng: lambda n: ft.libfm_rows(rng, n, 30),
            e=lambda rng, nb: ft.dense_libfm(rng, nb),
            violate=b"1 1:2:3:4", error=(b"1 -3:4:5", 2, ERR_NEG_INDEX)),
        "csv_tab_i64": dict(
            fmt=po.CSV, kw={"label_column": 0, "delimiter": "\t", "value_type": 2}, delim=b"\t", nchunks=3, seed=5400,
            a=lambda rng: lambda n: _int_csv(rng, n, 9, "\t"),
            b=lambda rng: lambda n: _int_csv(rng, n, 28, "\t"),
            e=lambda rng, nb: _short_csv(rng, nb, 12, "\t"),
            violate=b"\t".join([b"1", b"25", b"-3"] + [b"7"] * 5 + [b" "]), error=(b"5", 1, ERR_CSV_DELIM)),
    }


FAMILIES = ("libsvm", "csv", "libfm", "csv_tab_i64")
_CACHE = {}


def family(name, tile):
    """{"fmt", "kw", "nbytes", "nchunks", "members": {name: member}}; a member
    is {"name", "data", "offs", "expect"} plus, for D, "err": (code, byte
    position) and, for C and D, "at": the placed line's position."""
    key = (name, tile)
    if key in _CACHE:
        return _CACHE[key]
    s = _specs()[name]
    rng = np.random.default_rng(s["seed"])
    nbytes, delim, nch = 3 * tile + REM, s["delim"], s["nchunks"]
    la = split_lines(fc.grown(s["a"](rng), nbytes + 2000))
    lb = split_lines(fc.grown(s["b"](rng), nbytes + 4000))
    le = split_lines(s["e"](rng, nbytes + 4000))
    mid = tile + tile // 2
    lc, at_c = with_line(la, s["violate"], mid)
    eline, eoff, ecode = s["error"]
    ld, at_d = with_line(la, eline, mid)
    assert tile <= at_c and at_c + len(s["violate"]) < 2 * tile
    frac = lambda k: [nbytes * (i + 1) // k for i in range(nch - 1)]  # noqa: E731
    members = {}
    # (B's chunks start at other lines than A's: fifths instead of equal parts)
    for m, lines, targets, expect in (("A", la, frac(nch), "stay"), ("B", lb, frac(nch + 2), "stay"),
                                      ("C", lc, frac(nch), "hand"), ("D", ld, frac(nch), "error"),
                                      ("E", le, frac(nch + 1), "capacity")):
        lines = fit(lines, nbytes, delim)
        members[m] = {"name": m, "data": b"".join(lines), "offs": cuts_near(lines, targets), "expect": expect}
    members["C"]["at"] = at_c
    members["D"]["at"] = at_d
    members["D"]["err"] = (ecode, at_d + eoff)
    fam = {"name": name, "fmt": s["fmt"], "kw": dict(s["kw"]), "nbytes": nbytes, "nchunks": nch, "members": members,
           "violate": s["violate"], "error_line": eline}
    _CACHE[key] = fam
    return fam


# parse graphs: configuration -> (family, parser keywords on top of the family's)
FLAG_EXACT, FLAG_MAX_INDEX = fc.FLAG_EXACT, fc.FLAG_MAX_INDEX
CONFIGS = {
    "libsvm_max_index": ("libsvm", {"flags": FLAG_MAX_INDEX}),
    "csv_max_index": ("csv", {"flags": FLAG_MAX_INDEX}),
    "libfm_max_index": ("libfm", {"flags": FLAG_MAX_INDEX}),
    "libsvm_auto_index_nthread2": ("libsvm", {"indexing_mode": -1, "nthread": 2}),
    "csv_tab_i64_label0": ("csv_tab_i64", {}),
    "libsvm_exact": ("libsvm", {"flags": FLAG_EXACT}),
}


def config_kw(config):
    """(family name, DeviceParser keywords) of a parse-graph configuration."""
    name, extra = CONFIGS[config]
    kw = dict(_specs()[name]["kw"])
    kw.update(extra)
    return name, kw


def oracle_of(fam, member, kw):
    """The oracle's result for a member under DeviceParser keywords kw."""
    okw = {("value_kind" if k == "value_type" else k): v for k, v in kw.items() if k != "flags"}
    m = fam["members"][member]
    return po.parse_chunks(m["data"], m["offs"], fmt=fam["fmt"], **okw)


def captured_caps(oracles):
    """The seven capacities a graph is captured with: the slot-wise maximum of
    the oracle's counts over A, B and C, plus SLACK."""
    return [max(fc.oracle_counts(oracles[m])[s] for m in "ABC") + SLACK for s in range(7)]


# -------------------------------------------------------------- chain --
CHAIN_NCOL = 257     # feature columns: two 8-bit column digits in to_csc and make_cuts
CHAIN_MAX_BIN = 16
CHAIN_SAMPLE = 400   # make_cuts's max_rows: a sample of the gathered rows
CHAIN_KW = {"label_column": 0, "flags": FLAG_MAX_INDEX}
CHAIN_ORDER = (("A", 1), ("B", 1), ("A", 2), ("D", 1), ("A2", 1), ("A", 1))
SENT = 0xA5          # every byte of a post-parse output before a replay
GUARD = 3            # guard elements (rows, for the matrices) behind every post-parse output
NAN_BITS = 0x7FC00000


def _chain_rows(rng, nrows, every, narrow):
    """CSV rows "label,v,v,...": each `every`-th row holds all 257 feature
    columns, the others `narrow`; every value is d.ddd (5 bytes)."""
    out = []
    levels = rng.integers(2, 12, size=CHAIN_NCOL)  # every third column holds few distinct values: fewer cuts than max_bin
    few = np.arange(CHAIN_NCOL) % 3 == 0
    for r in range(nrows):
        n = CHAIN_NCOL if r % every == 0 else narrow
        v = rng.integers(0, 10000, size=n)
        v = np.where(few[:n], v % levels[:n] * 777, v)
        out.append(b"%d," % int(rng.integers(0, 2)) + b",".join(b"%d.%03d" % (x // 1000, x % 1000) for x in v) + b"\n")
    return out


def chain_family(geom):
    """geom: {"csc", "cuts": entries per tile; "gather": ids per tile;
    "dense", "bins": (cells per tile, rows per tile)}.  -> {"members": {A, B,
    D, A2}, "ids": {1: a permutation prefix, 2: repeats and one bad id},
    "nbytes", "nchunks", "n_ids"}.  More than two tiles of ids for
    gather_rows, of rows for to_dense / to_bins, of entries for to_csc and for
    the sample make_cuts reads."""
    key = ("chain", tuple(sorted((k, tuple(np.atleast_1d(v).tolist())) for k, v in geom.items())))
    if key in _CACHE:
        return _CACHE[key]
    rng = np.random.default_rng(5500)
    n_ids = 2 * geom["gather"] + 9
    rows_a = n_ids + 40
    la = _chain_rows(rng, rows_a, 8, 16)
    nbytes = sum(len(x) for x in la)
    lb = fit(_chain_rows(rng, 2 * rows_a, 12, 20), nbytes, b",", can_pad=lambda x: len(x) < 400)
    ld, at_d = with_line(la, b"5", nbytes // 2)
    ld = fit(ld, nbytes, b",", can_pad=lambda x: len(x) < 400)
    a2 = bytearray(b"".join(la))
    dots = np.flatnonzero(np.frombuffer(bytes(a2), dtype=np.uint8) == ord("."))
    for p in dots[::3]:  # a third of the values move: the digit before the point and the one after it
        a2[p - 1] = ord("0") + (a2[p - 1] - ord("0") + 3) % 10
        a2[p + 1] = ord("0") + (a2[p + 1] - ord("0") + 7) % 10
    members = {}
    for m, data, lines, k in (("A", b"".join(la), la, 3), ("B", b"".join(lb), lb, 5), ("D", b"".join(ld), ld, 3),
                              ("A2", bytes(a2), la, 3)):
        members[m] = {"name": m, "data": data, "offs": cuts_near(lines, [nbytes * (i + 1) // k for i in range(2)]),
                      "expect": "error" if m == "D" else "ok"}
    members["D"]["err"] = (ERR_CSV_DELIM, at_d + 1)
    ids1 = rng.permutation(rows_a)[:n_ids].astype(np.int64)
    ids2 = rng.integers(0, rows_a // 2, size=n_ids).astype(np.int64)  # every id about twice
    ids2[n_ids // 3] = (1 << 32) + 1
    fam = {"members": members, "ids": {1: ids1, 2: ids2}, "nbytes": nbytes, "nchunks": 3, "n_ids": n_ids,
           "fmt": po.CSV, "kw": dict(CHAIN_KW)}
    _CACHE[key] = fam
    return fam


def chain_oracle(fam, member):
    return oracle_of(fam, member, fam["kw"])


def chain_dims(fam, oracles):
    """Host arguments frozen into the chain graph: the capacities of the
    parse's outputs (upper bounds over the members) and of the gather's (the
    largest gather of the replay order), and the cut capacity."""
    ok = [o for o in oracles.values() if o["status"] == 0]
    rows = max(len(o["offset"]) - 1 for o in ok) + 50
    nnz = max(len(o["index"]) for o in ok) + 50
    ent = 0
    for m, which in CHAIN_ORDER:
        o = oracles[m]
        if o["status"] == 0:
            off = o["offset"].astype(np.int64)
            ids = fam["ids"][which]
            good = ids[(ids >= 0) & (ids < len(off) - 1)]
            ent = max(ent, int((off[good + 1] - off[good]).sum()))
    return {"rows": rows, "nnz": nnz, "g_rows": fam["n_ids"] + GUARD, "g_ent": ent + 50, "ncol": CHAIN_NCOL,
            "cut_cap": CHAIN_NCOL * CHAIN_MAX_BIN, "n_ids": fam["n_ids"]}


def _sent(n, dtype):
    return np.frombuffer(bytes([SENT]) * (int(n) * np.dtype(dtype).itemsize), dtype=dtype).copy()


def chain_expect(o, err, ids, d):
    """What the six calls leave behind, by the models over the oracle's CSR
    `o` (err: the parse's error word when the oracle raises): every output
    buffer, guard elements included, as the caller pre-filled it with SENT,
    and every result and status block.  Arrays are unsigned words."""
    n_ids, ncol, ge, gr = d["n_ids"], d["ncol"], d["g_ent"], d["g_rows"]
    res = np.zeros(16, dtype=U64)
    if err:
        res[8] = err
        side = gm.side_from({"offset": np.zeros(1, U64), "label": np.zeros(0, U32), "index": np.zeros(0, U32),
                             "value": np.zeros(0, U32)}, {gm.ROWS: d["rows"], gm.INDEX: d["nnz"], gm.VALUE: d["nnz"]})
    else:
        rows, nnz = len(o["offset"]) - 1, len(o["index"])
        res[gm.ROWS] = res[gm.LABEL] = rows
        res[gm.INDEX] = res[gm.VALUE] = nnz
        res[10] = int(np.asarray(o["index"]).max())
        side = gm.side_from({"offset": np.asarray(o["offset"]).astype(U64), "label": gm.bits(np.asarray(o["label"], np.float32)),
                             "index": np.asarray(o["index"]).astype(U32), "value": gm.bits(np.asarray(o["value"], np.float32))},
                            {gm.ROWS: d["rows"], gm.INDEX: d["nnz"], gm.VALUE: d["nnz"]})
    dst = gm.side_from({"offset": _sent(gr + 1 + GUARD, U64), "label": _sent(gr + GUARD, U32), "weight": _sent(gr + GUARD, U32),
                        "qid": _sent(gr + GUARD, U64), "field": _sent(ge + GUARD, U32), "index": _sent(ge + GUARD, U32),
                        "value": _sent(ge + GUARD, U32)},
                       {gm.ROWS: gr, gm.WEIGHT: gr, gm.QID: gr, gm.FIELD: ge, gm.INDEX: ge, gm.VALUE: ge})
    g, gres, gst = gm.gather_rows(side, res, ids.astype(np.int64).view(U64), dst, max_index=True)
    want = {"g_" + k: g[k] for k in gm.ARRAYS}
    want["g_res"] = np.array(gres[:12], dtype=U64)
    want["g_status"] = np.array(gst, dtype=U64)
    gerr = int(gres[8])
    counts = (int(gres[gm.ROWS]), int(gres[gm.INDEX]), int(gres[gm.VALUE]))
    common = dict(counts=counts, ncol=ncol, error=gerr, cap_rows=gr, cap_index=ge)
    goff, gidx, gval = g["offset"], g["index"], g["value"]
    cuts, cst = qm.make_cuts(goff, gidx, gval, {"cut_ptr": _sent(ncol + 1 + GUARD, U32),
                                                "cut_value": _sent(d["cut_cap"] + GUARD, U32), "cap": d["cut_cap"]},
                             max_bin=CHAIN_MAX_BIN, cap_value=ge, max_rows=CHAIN_SAMPLE, **common)
    want["cut_ptr"], want["cut_value"], want["cuts_status"] = cuts["cut_ptr"], cuts["cut_value"], np.array(cst, dtype=U64)
    bins, bst = bm.to_bins(goff, gidx, gval.view(np.float32), _sent((n_ids + GUARD) * ncol, np.uint8), cuts["cut_ptr"],
                           cuts["cut_value"].view(np.float32), n_cuts=d["cut_cap"], **common)
    want["bins"], want["bins_status"] = bins, np.array(bst, dtype=U64)
    dense, dst4 = dmod.to_dense(goff, gidx, gval, _sent((n_ids + GUARD) * ncol, U32), value_dtype=np.float32,
                                fill_bits=NAN_BITS, **common)
    want["dense"], want["dense_status"] = dense, np.array(dst4, dtype=U64)
    csc, sst = cm.to_csc(goff, gidx, gval, {"col_offset": _sent(ncol + 1 + GUARD, U64), "row": _sent(ge + GUARD, U32),
                                           "value": _sent(ge + GUARD, U32), "pos": _sent(ge + GUARD, U64), "cap": ge},
                         cap_value=ge, **common)
    for k in ("col_offset", "row", "value", "pos"):
        want["csc_" + k] = csc[k]
    want["csc_status"] = np.array(sst, dtype=U64)
    return want
