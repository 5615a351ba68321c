"""TEST INFRASTRUCTURE ONLY -- the inputs of tests/test_gpu_numbers.py: the
number catalogue (tests/numcat.py) placed in every numeric role of libsvm,
libfm and CSV text, and at every alignment.

A case is a dict: name, fmt, data, offs, kw (parser keywords), expect ("stay":
the single pass must keep it, "hand": it must hand over, None), parsed (the
oracle must parse it, so the arrays are compared), err (the error code both
must raise, or None), numbers / window / byte (catalogue entries placed and
their tags).  run_case() sends one through tests/full_call.full_vs_oracle.

Whether a line of digit characters is a row the reference can take -- "1 3:+"
is, "1 3:1..2" leaves a feature without a value, which fails its whole chunk
-- is decided by the oracle, line by line (line_ok, as full_call.valued_lines):
the lines it rejects go to an input of their own, compared by failure status.
"""
import ctypes

import numpy as np

import numcat
from oracle import pyoracle as po

ERR_NEG_INDEX, ERR_NAN_LITERAL = 1, 2
FLAG_EXACT = 4


# ----------------------------------------------------------------- helpers --
def line_ok(lines, fmt, weight=False, **okw):
    """Per line: parsed behind a '\\n' on its own, the reference neither raises
    nor leaves a feature without a value, nor a row without the label or the
    weight the role is about (a CSV field that ParseFloat consumes nothing of
    is a missing one)."""
    L = po.oracle_lib()
    prm = po.params(fmt=fmt, **okw)
    weight = weight or prm.weight_column >= 0
    out = []
    for line in lines:
        raw = line.encode("latin-1") if isinstance(line, str) else line
        buf = ctypes.create_string_buffer(b"\n" + raw + b"\n", len(raw) + 3)
        c = po.Csr()
        L.dmo_csr_init(ctypes.byref(c), prm.value_kind)
        L.dmo_parse_block(ctypes.cast(buf, ctypes.c_void_p), len(raw) + 2, ctypes.byref(prm), ctypes.byref(c))
        out.append(c.status == 0 and c.n_index == c.n_value and c.n_rows == 1 and (not weight or c.n_weight == 1)
                   and (prm.label_column < 0 or c.n_label == 1))
        L.dmo_csr_free(ctypes.byref(c))
    return out


def line_cuts(data, n):
    """[0, about n cuts after a newline, len(data)]."""
    a = np.frombuffer(data, dtype=np.uint8)
    nl = np.flatnonzero(a == 10) + 1
    nl = nl[nl < len(data)]
    if len(nl) == 0 or n == 0:
        return [0, len(data)]
    pick = nl[np.linspace(0, len(nl) - 1, n + 2).astype(int)[1:-1]]
    return [0] + sorted(set(int(x) for x in pick)) + [len(data)]


def _case(name, fmt, lines, kw=None, expect=None, parsed=False, err=None, entries=(), kind="float", cuts=3,
          tail=True):
    data = "\n".join(lines).encode("latin-1") + (b"\n" if tail and lines else b"")
    tags = [numcat.EXPECT[kind](s) for s in entries]
    return {"name": name, "fmt": fmt, "data": data, "offs": line_cuts(data, cuts), "kw": dict(kw or {}),
            "expect": expect, "parsed": parsed, "err": err, "numbers": len(entries),
            "window": tags.count("window"), "byte": tags.count("byte")}


def run_case(dm, fc, c, exact=False):
    """One full call against the oracle; asserts the path, the parse status and the error code."""
    kw = dict(c["kw"])
    if exact:
        kw["exact"] = True
    prm = dm.make_params(fc.FMT_NAME[c["fmt"]], **{k: v for k, v in kw.items() if k != "exact"})
    o = po.parse_chunks(c["data"], c["offs"], fmt=c["fmt"], **fc.oracle_kw(prm))
    try:
        if c["parsed"]:
            assert o["status"] == 0, o["msg"]
        if c["err"] is not None:
            assert o["status"] != 0, "the oracle parsed an input built to raise"
        h = fc.full_vs_oracle(dm, c["data"], c["offs"], c["fmt"], oracle=o, slack=7, **kw)
        if c["err"] is not None:
            assert dm.error_code(h["error"]) == c["err"], (h["error"], o["msg"])
        if exact:
            assert h["path"] != 0, h["path"]
        elif c["expect"] == "stay":
            assert h["path"] == 0, h["path"]
        elif c["expect"] == "hand":
            assert h["path"] != 0 or h["error"] != 0, h["path"]
    except AssertionError as e:
        raise AssertionError("%s kw=%s exact=%s: %s" % (c["name"], kw, exact, str(e)[:1500]))
    return h


# ------------------------------------------------------- value role, dense --
def _rows(strs, per, one, sep, head):
    n = len(strs)
    pad = (-n) % per
    strs = list(strs) + ["1"] * pad
    cells = [one(i % per, s) for i, s in enumerate(strs)]
    return [head + sep.join(cells[i:i + per]) for i in range(0, len(cells), per)]


def svm_value_rows(strs, per=8):
    return _rows(strs, per, lambda j, s: "%d:%s" % (3 + 4 * j, s), " ", "1 ")


def fm_value_rows(strs, per=8):
    return _rows(strs, per, lambda j, s: "%d:%d:%s" % (j + 1, 3 + 4 * j, s), " ", "1 ")


def csv_value_rows(strs, per=8, delim=","):
    return _rows(strs, per, lambda j, s: s, delim, "")


def dense_strings():
    """frac_exhaustive and the full midpoint class: 397 330 strings, all window."""
    out = []
    for _, arr in numcat.frac_exhaustive():
        out += arr.tolist()
    return out + numcat.catalogue(False).pick(kind="float", cls="midpoint")


def dense_cases():
    strs = dense_strings()
    out = []
    for fmt, name, rows in ((po.LIBSVM, "libsvm", svm_value_rows), (po.CSV, "csv", csv_value_rows),
                            (po.LIBFM, "libfm", fm_value_rows)):
        out.append(_case("dense_value_" + name, fmt, rows(strs), expect="stay", parsed=True, entries=strs, cuts=5))
    return out


# -------------------------------------------------- every role, compact set --
def _split(name, fmt, kw, entries, line_of, kind, inside, okw=None, raises=(), err=None, alone=False, cuts=3,
           weight=False, alone_expect=None):
    """The two halves of a role: the entries inside the kernel's grammar that
    the reference takes (stay, arrays compared) and the rest -- the lines the
    reference rejects together (failure status compared), the entries outside
    the grammar (together: handed over, arrays compared; alone=True: each
    behind clean lines, whatever the reference makes of it -- the libsvm and
    libfm tokenizers never hand a letter to ParseFloat, so "3:inf" is a
    feature without a value and "nan(" raises nothing; alone_expect is their
    path: libfm's single pass hands every line with a letter over, libsvm's
    walks such lines itself (svm_fast.h dirty lines) and keeps those the
    reference parses, so there only the arrays are compared), and each entry that
    raises alone behind clean lines (the error code compared)."""
    ins = [s for s in entries if inside(s) and s not in raises]
    ok = line_ok([line_of(s) for s in ins], fmt, weight=weight, **(okw or {}))
    keep = [s for s, k in zip(ins, ok) if k]
    drop = [s for s, k in zip(ins, ok) if not k]
    # the oracle's filter may only take malformed numbers away (it cannot hollow the role)
    assert all(s in numcat.DEGENERATE or s in numcat.LETTERS for s in drop), (name, drop[:10])
    out = [_case(name + "/in", fmt, [line_of(s) for s in keep], kw, "stay", True, entries=keep, kind=kind, cuts=cuts)]
    if drop:
        out.append(_case(name + "/rejected", fmt, [line_of(s) for s in drop], kw, None, False, entries=drop, kind=kind,
                         cuts=0))
    outside = [s for s in entries if not inside(s) and s not in raises]
    if outside and alone:
        for s in outside:
            out.append(_case(name + "/outside:" + s, fmt, [line_of(x) for x in keep[:20] + [s] + keep[:20]], kw,
                             alone_expect, False, entries=[s], kind=kind, cuts=0))
    elif outside:
        out.append(_case(name + "/outside", fmt, [line_of(s) for s in keep[:40] + outside + keep[:40]], kw, "hand",
                         True, entries=outside, kind=kind, cuts=1))
    for s in raises:
        if s in entries:
            out.append(_case(name + "/raises:" + s, fmt, [line_of(x) for x in keep[:20] + [s] + keep[:20]], kw, None,
                             False, err=err, entries=[s], kind=kind, cuts=0))
    return out


def qid_strings():
    """1-18 digits (the single pass reads them), then 19 and more."""
    pat = "1234567890123456789012345"
    short = [pat[:n] for n in range(1, 19)] + ["9" * n for n in (7, 8, 9, 10, 16, 17, 18)] + \
        ["0", "00000005", "0000000000000005", "4294967295", "4294967296"]
    return short, [pat[:19], pat[:20], "9" * 19, "18446744073709551615", "18446744073709551616", "0" * 19 + "5"]


def role_cases():
    cat = numcat.catalogue(True)
    F = cat.pick(kind="float")
    I = cat.pick(kind="index")
    N = cat.pick(kind="int")
    G = numcat.in_grammar
    nan_raises = numcat.RAISES
    neg = tuple(s for s in I if s.startswith("-"))
    out = []
    # ---- libsvm
    for role, line_of in (("label", lambda s: s + " 3:1 7:0.5"), ("weight", lambda s: "1:" + s + " 3:1 7:0.5"),
                          ("value", lambda s: "1 3:" + s + " 7:0.5")):
        out += _split("libsvm_" + role, po.LIBSVM, {}, F, line_of, "float", G, alone=True, weight=role == "weight")
    for bits in (32, 64):
        for im, nt in ((0, 1), (1, 2), (-1, 1), (-1, 2), (0, 2), (1, 1)):
            kw = {"index_bits": bits, "indexing_mode": im, "nthread": nt}
            okw = {"index_bits": bits, "indexing_mode": im}
            out += _split("libsvm_index_b%d_im%d_t%d" % (bits, im, nt), po.LIBSVM, kw, I,
                          lambda s: "1 " + s + ":1 70:0.5", "index", G, okw=okw, raises=neg, err=ERR_NEG_INDEX)
    short, long_ = qid_strings()
    out.append(_case("libsvm_qid/in", po.LIBSVM, ["1 qid:%s 3:1" % q for q in short], {}, "stay", True, entries=short,
                     kind="index"))
    out.append(_case("libsvm_qid/long", po.LIBSVM, ["1 qid:%s 3:1" % q for q in short[:20] + long_ + short[:20]], {},
                     "hand", True, entries=long_, kind="index", cuts=1))
    # ---- libfm
    for role, line_of in (("label", lambda s: s + " 1:3:1 2:7:0.5"), ("value", lambda s: "1 1:3:" + s + " 2:7:0.5")):
        out += _split("libfm_" + role, po.LIBFM, {}, F, line_of, "float", G, alone=True, alone_expect="hand")
    for role, line_of in (("field", lambda s: "1 " + s + ":3:1 2:7:0.5"), ("index", lambda s: "1 1:" + s + ":1 2:7:0.5")):
        for bits in (32, 64):
            out += _split("libfm_%s_b%d" % (role, bits), po.LIBFM, {"index_bits": bits}, I, line_of, "index", G,
                          okw={"index_bits": bits}, raises=neg, err=ERR_NEG_INDEX)
    # ---- CSV, float values: letters are inside its grammar
    everything = lambda s: True  # noqa: E731
    for name, kw, line_of in (
            ("csv_field", {}, lambda s: "1," + s + ",0.5"),
            ("csv_field_last", {}, lambda s: "1,0.5," + s),
            ("csv_label0", {"label_column": 0}, lambda s: s + ",1,0.5"),
            ("csv_label_last", {"label_column": 2}, lambda s: "1,0.5," + s),
            ("csv_weight", {"weight_column": 1}, lambda s: "1," + s + ",0.5"),
            ("csv_label_weight", {"label_column": 0, "weight_column": 2}, lambda s: s + ",1," + s),
            ("tsv_field", {"delimiter": "\t"}, lambda s: "1\t" + s + "\t0.5")):
        okw = {k: v for k, v in kw.items()}
        out += _split(name, po.CSV, kw, F, line_of, "float", everything, okw=okw, raises=nan_raises,
                      err=ERR_NAN_LITERAL)
    # ---- CSV, integer values: strtoll base 0; digits and a sign are inside the grammar
    digits = lambda s: all(c in "0123456789+-" for c in s)  # noqa: E731
    for vt, vname in ((1, "i32"), (2, "i64")):
        for dname, d in (("comma", ","), ("tab", "\t")):
            for lname, lc, line_of in (("value", -1, lambda s, d=d: "1" + d + s + d + "5"),
                                       ("last", -1, lambda s, d=d: "1" + d + "5" + d + s),
                                       ("label0", 0, lambda s, d=d: s + d + "1" + d + "5")):
                kw = {"value_type": vt, "delimiter": d}
                if lc >= 0:
                    kw["label_column"] = lc
                okw = {"value_kind": vt, "delimiter": d, "label_column": lc}
                out += _split("csv_%s_%s_%s" % (vname, dname, lname), po.CSV, kw, N, line_of, "int", digits, okw=okw)
    return out


# ------------------------------------------------------------ alignment --
def sweep_entries(nmid=200):
    cat = numcat.catalogue(True)
    mid = cat.pick(kind="float", cls="midpoint")
    return cat.pick(kind="float", cls=("boundary", "degenerate")) + mid[::max(len(mid) // nmid, 1)][:nmid]


def _valued(entries, fmt, line_of):
    ok = line_ok([line_of(s) for s in entries], fmt)
    return [s for s, k in zip(entries, ok) if k]


def align_svm(entries):
    """Each entry as a libsvm value with its first byte at every offset 0..63
    modulo 64 (blanks before the index pad the row).  Returns (case, starts):
    starts[i] lists the byte offsets of entry i."""
    entries = _valued(entries, po.LIBSVM, lambda s: "1 3:" + s)
    parts, pos, starts = [], 0, [[] for _ in entries]
    for r in range(64):
        for i, s in enumerate(entries):
            nb = (r - (pos + 1 + 3)) % 64
            row = "1" + " " * nb + " 3:" + s + ("\n" if (i + r) % 2 else " 7:1\n")
            starts[i].append(pos + 1 + nb + 3)
            parts.append(row)
            pos += len(row)
    data = "".join(parts).encode("latin-1")
    c = _case("align_libsvm", po.LIBSVM, [], expect="stay", parsed=True, entries=entries * 64)
    c["data"], c["offs"] = data, line_cuts(data, 4)
    return c, entries, starts


def align_csv(entries):
    """The same as a CSV field behind short fields ("1," and one "12," for parity)."""
    entries = _valued(entries, po.CSV, lambda s: "1," + s)
    parts, pos, starts = [], 0, [[] for _ in entries]
    for r in range(64):
        for i, s in enumerate(entries):
            gap = (r - pos) % 64
            if gap == 1:
                gap += 64
            pre = ("12," if gap % 2 else "") + "1," * ((gap - (3 if gap % 2 else 0)) // 2)
            row = pre + s + ("\n" if (i + r) % 2 else ",7\n")
            starts[i].append(pos + len(pre))
            parts.append(row)
            pos += len(row)
    data = "".join(parts).encode("latin-1")
    c = _case("align_csv", po.CSV, [], expect="stay", parsed=True, entries=entries * 64)
    c["data"], c["offs"] = data, line_cuts(data, 4)
    return c, entries, starts


def tile_end_svm(entries, tile):
    """Entry i as the last value of a row whose first byte lies 1 + i % 15
    bytes before the end of tile i + 1: filler rows, then one padded row."""
    entries = _valued(entries, po.LIBSVM, lambda s: "1 3:" + s)
    fill = "1 3:0.5 7:0.25 11:1 15:0.125 19:2 23:0.75 27:3 31:0.0625\n"
    parts, pos, starts = [], 0, []
    for i, s in enumerate(entries):
        target = (i + 1) * tile - (1 + i % 15)
        nfill = (target - pos - 70) // len(fill)
        parts.append(fill * nfill)
        pos += nfill * len(fill)
        nb = target - pos - 4
        assert 0 < nb < 70 + len(fill)
        row = "1" + " " * nb + " 3:" + s + "\n"
        starts.append(pos + 1 + nb + 3)
        parts.append(row)
        pos += len(row)
    data = "".join(parts).encode("latin-1")
    c = _case("tile_end_libsvm", po.LIBSVM, [], expect="stay", parsed=True, entries=entries)
    c["data"], c["offs"] = data, line_cuts(data, 4)
    return c, entries, starts


def tile_end_csv(entries, tile):
    entries = _valued(entries, po.CSV, lambda s: "1," + s)
    fill = "1,0.5,0.25,1,0.125,2,0.75,3,0.0625,12\n"
    parts, pos, starts = [], 0, []
    for i, s in enumerate(entries):
        target = (i + 1) * tile - (1 + i % 15)
        nfill = (target - pos - 50) // len(fill)
        parts.append(fill * nfill)
        pos += nfill * len(fill)
        gap = target - pos
        pre = ("12," if gap % 2 else "") + "1," * ((gap - (3 if gap % 2 else 0)) // 2)
        assert len(pre) == gap
        row = pre + s + "\n"
        starts.append(pos + gap)
        parts.append(row)
        pos += len(row)
    data = "".join(parts).encode("latin-1")
    c = _case("tile_end_csv", po.CSV, [], expect="stay", parsed=True, entries=entries)
    c["data"], c["offs"] = data, line_cuts(data, 4)
    return c, entries, starts


def chunk_end_cases(entries, tile, max_cs):
    """Entry i ends 1 + i % 15 bytes before a chunk start (blanks -- for CSV
    short fields -- then the newline the chunk is cut behind): a 16-byte window would pass its chunk.
    Filler rows keep the chunk starts of one tile below what the single pass
    takes (max_cs), so the input stays on it."""
    out = []
    gap = 2 * tile // max_cs + 64
    for fmt, name, pre, fill, blank_ok in ((po.LIBSVM, "libsvm", "1 3:", "1 3:0.5 7:0.25 11:1 15:0.125\n", True),
                                           (po.CSV, "csv", "1,", "1,0.5\n2,0.25\n", False)):
        ents = _valued(entries, fmt, lambda s: pre + s)
        parts, pos, offs, ends = [], 0, [0], []
        for i, s in enumerate(ents):
            g = i % 15
            if blank_ok:
                tail = " " * g
            else:  # (a blank behind a CSV number is part of its field: short fields follow it instead)
                g = 0 if g == 1 else g  # (one byte would be an empty field: CSV has distances 1 and 3..15)
                tail = ",1" * ((g - (3 if g % 2 else 0)) // 2) + (",12" if g % 2 else "")
            assert len(tail) == g
            row = fill * (gap // len(fill)) + pre + s + tail + "\n"
            parts.append(row)
            pos += len(row)
            ends.append(pos - 1 - g)
            offs.append(pos)
        c = _case("chunk_end_" + name, fmt, [], expect="stay", parsed=True, entries=ents)
        c["data"], c["offs"], c["ends"] = "".join(parts).encode("latin-1"), offs, ends
        out.append(c)
    return out


def text_end_cases(entries):
    """Each entry as the last bytes of a text, with and without a final newline."""
    out = []
    for fmt, name, pre in ((po.LIBSVM, "libsvm", "1 3:0.5\n1 7:"), (po.CSV, "csv", "1,0.5\n2,")):
        for s in _valued(entries, fmt, lambda s: pre.split("\n")[1] + s):
            for tail in (True, False):
                c = _case("text_end_%s:%s:%s" % (name, s, "nl" if tail else "eof"), fmt, [], parsed=True, entries=[s])
                c["data"] = (pre + s + ("\n" if tail else "")).encode("latin-1")
                c["offs"] = [0, len(c["data"])]
                out.append(c)
    return out
