"""CSV text generators for the float label / weight kernel of the single-pass
CSV family (csv_fast.h tile<MODE, true, 0, false>): header rows, text and
missing values, blanks and UTF-8 BOMs together with label_column /
weight_column.

The field at a special column is that column's entry whether or not ParseFloat
read anything: a header word, "NA" or an empty field there is a label (weight)
of 0.  A weight that reads as NaN is a missing weight and leaves the single
pass, as does a row that does not reach a special column.

headers(), text(), blanks(), boms(): inside the single-pass grammar by
construction.  With a special column past column 0 a row that holds a
tokenless field (empty, or text ParseFloat does not read) must not cross a
tile boundary -- a tile cannot know such a field's column before its
look-back -- so the generators rewrite a crossing row as plain
numbers; label_column=0 alone has no such rule.
edge_cases(): hand-placed inputs, each with a flag saying whether it must stay
on the single pass.  violations(): outside it; the exact kernels.
"""
import numpy as np

from fuzz_ws import TILE

BOM = "\xef\xbb\xbf"
# (label_column, weight_column); "last" = the last column of the input
FORMS = [(0, -1), (1, -1), ("last", -1), (0, 2), (3, 1)]
CLASSES = ["headers", "text", "blanks", "boms"]

# names that start with 'f' / 'i' / 'n' (ParseFloat's suffix and the first
# letters of inf / nan) and names that spell inf... / nan...
NAMES = ["label", "y", "target", "f0", "f1", "feature_2", "F", "id", "index", "income", "Info", "inf", "infinity_x",
         "infinit", "n_items", "name", "nanny", "nan_count", "NaN", "x1", "col 7", "weight", "w", "\xe9t\xe9", "e5", "-"]
WORDS = ["NA", "?", "", "nan", "-inf", "Infinity", "3.5kg", "N/A", "null", "abc", "+NAN", "inF", "-", "fin", "in"]


def _reads_nan(s):
    return s.strip(" \t").lstrip("+-").lower().startswith("nan")


def resolve(form, ncols):
    lc, wc = form
    return (ncols - 1 if lc == "last" else lc), wc


def _num(rng):
    r = rng.random()
    if r < 0.6:
        return "%.9g" % (rng.random() * 2 - 1)
    if r < 0.9:
        return str(int(rng.integers(0, 1000)))
    return ["1e5", "-.5", "007", "2.5e-3", "+7", "123456789.125"][int(rng.integers(0, 6))]


def _plain_row(rng, ncols, lc):
    f = [_num(rng) for _ in range(ncols)]
    f[lc] = str(int(rng.integers(0, 2)))
    return ",".join(f)


def _header(rng, ncols, wc):
    f = [NAMES[int(rng.integers(0, len(NAMES)))] for _ in range(ncols)]
    if wc >= 0 and _reads_nan(f[wc]):
        f[wc] = "weight"  # a weight that reads as NaN is a missing weight: outside the grammar
    return ",".join(f)


def _field(rng, cls, j, ncols, lc, wc):
    """One field of a body row; the last field never ends in a blank run or is
    empty (the decoder would read on into the next line / no phantom field)."""
    special = j in (lc, wc)
    last = j == ncols - 1
    v = str(int(rng.integers(0, 3))) if special and rng.random() < 0.5 else _num(rng)
    if cls in ("text", "boms") and rng.random() < (0.35 if special else 0.15):
        v = WORDS[int(rng.integers(0, len(WORDS)))]
        if j == wc and _reads_nan(v):
            v = "NA"
        if last and v == "":
            v = "?"
    if cls == "blanks":
        r = rng.random()
        if r < 0.12 and not last:
            return " " * int(rng.integers(1, 4))  # a blank field ending at a delimiter: ParseFloat's 0
        if r < 0.22:
            v = ["NA", "abc", "inf", "x"][int(rng.integers(0, 4))]  # blanks running into text: a 0 (or inf)
        pad = " " * int(rng.integers(1, 3)) if (j > 0 or rng.random() < 0.3) and rng.random() < 0.8 else ""
        v = pad + ("\t" if rng.random() < 0.1 else "") + v
        if not last and rng.random() < 0.15:
            v += " "
    return v


def gen(rng, cls, nlines, form, ncols=None, eols=None):
    """(data, label_column, weight_column): `nlines` rows of `ncols` fields."""
    lo = max(2, max(c for c in form if c != "last") + 2)
    ncols = ncols or int(rng.integers(lo, lo + 8))
    lc, wc = resolve(form, ncols)
    M = max(lc, wc)
    eols = eols or ["\n"] * 10 + ["\r\n", "\n\n"]
    period = max(2, nlines // 4)  # a header row at the text start and at "file" starts
    out, pos = [], 0
    for i in range(nlines):
        bom = ""
        if cls in ("headers", "boms") and i % period == 0:
            row = _header(rng, ncols, wc)
            if cls == "boms" and rng.random() < 0.7:
                bom = BOM
        else:
            row = ",".join(_field(rng, cls, j, ncols, lc, wc) for j in range(ncols))
            if cls == "boms" and (i == 0 or rng.random() < 0.1):
                bom = BOM  # in front of a number, a word or blanks
        row = bom + row
        if M >= 1 and pos // TILE != (pos + len(row.encode("latin-1"))) // TILE:
            row = _plain_row(rng, ncols, lc)
        row += eols[int(rng.integers(0, len(eols)))]
        out.append(row)
        pos += len(row)
    return "".join(out).encode("latin-1"), lc, wc


def bom_cuts(data):
    """Chunk offsets with a cut at every row-start BOM after the first row."""
    b = BOM.encode("latin-1")
    cuts = [i for i in range(1, len(data)) if data.startswith(b, i) and data[i - 1:i] in (b"\n", b"\r")]
    return [0] + cuts + [len(data)]


def sized(rng, cls, form, nbytes, ncols=12):
    """About nbytes of class `cls`, ending at a line end."""
    n = 64
    data, lc, wc = gen(rng, cls, n, form, ncols)
    while len(data) < nbytes:
        n *= 2
        data, lc, wc = gen(rng, cls, n, form, ncols)
    k = data.index(b"\n", nbytes - 60) + 1
    return data[:k], lc, wc


def _fill(n, delim=","):
    """Exactly n bytes of short numeric rows (n = 0 or n >= 4)."""
    if n == 0:
        return ""
    assert n >= 4, n
    k = (n - 4) // 4
    return ("1%s2\n" % delim) * k + "1" + delim + "3" * (n - 4 * k - 3) + "\n"


def carried_field(k, what, ncols):
    """A row that starts before the tile boundary with a tokenless field `what`
    exactly k delimiters after the tile start."""
    head = ",".join(str(i % 10) for i in range(ncols))  # the columns before the tile: past any special column
    pre = _fill(TILE - len(head) - 1) + head + ","  # the boundary falls right after this delimiter
    assert len(pre) == TILE
    return (pre + "".join("5," for _ in range(k)) + what + ",6,7\n1,2,3,4,5\n").encode("latin-1")


def bom_blanks(n, delta, delim=",", bnd=None):
    """A row-start BOM, n blanks, then a number whose first byte stands at
    `delta` bytes after a 64-byte segment boundary."""
    bnd = bnd or 64 * ((n + 3 + 8 + 63) // 64) + 64
    pre = _fill(bnd + delta - n - 3, delim)
    blank = " "
    return (pre + BOM + blank * n + "5%s6%s7\n8%s9%s1\n" % ((delim,) * 4)).encode("latin-1")


def edge_cases():
    """[(name, data, label_column, weight_column, delimiter, fast)]; fast: True =
    must stay on the single pass, None = either path."""
    c = []
    # tokenless special fields in a row carried into a tile, 0, 1, M and M + 1 delimiters after its start
    for lc, wc in ((1, -1), (3, 1), (0, 2), (0, -1)):
        M = max(lc, wc)
        for k in sorted({0, 1, M, M + 1}):
            for what in ("", "NA"):
                c.append(("carried_l%d_w%d_k%d_%s" % (lc, wc, k, what or "empty"), carried_field(k, what, 3),
                          lc, wc, ",", True if M == 0 else None))
    # the same row when the tile knows its start: the tile begins with the row
    c.append(("row_at_tile_start", (_fill(TILE) + "1,,NA,4\n1,NA,3,4\n").encode("latin-1"), 1, -1, ",", True))
    # a label field cut by a segment boundary and by a tile boundary: a number, a word
    for bnd in (64, TILE):
        for lab in ("12345", "label", " NA"):
            for split in (1, 2):
                pre = _fill(bnd - 2 - split)
                c.append(("label_cut_%d_%s_%d" % (bnd, lab.strip(), split), (pre + "7," + lab + ",8\n1,2,3\n").encode("latin-1"),
                          1, -1, ",", None))
                c.append(("label0_cut_%d_%s_%d" % (bnd, lab.strip(), split),
                          (_fill(bnd - split) + lab + ",8\n1,2\n").encode("latin-1"), 0, -1, ",", True))
    # a header longer than a tile; label_column=0 alone: a row of text fields of any length
    hdr = ",".join("name_%d" % i for i in range(2200)) + "\n"
    assert len(hdr) > TILE + 4000
    body = ",".join("1" for _ in range(2200)) + "\n"
    c.append(("long_header_label0", (hdr + body).encode("latin-1"), 0, -1, ",", True))
    c.append(("long_header_label5", (hdr + body).encode("latin-1"), 5, -1, ",", None))
    c.append(("long_header_label_w", (hdr + body).encode("latin-1"), 3, 1, ",", None))
    c.append(("crlf", b"label,f0,w\r\n1,2.5,3\r\n\r\n0,,4\r\nNA,?,\r\n", 0, 2, ",", None))
    c.append(("crlf_fast", b"label,f0,w\r\n1,2.5,3\r\n\r\n0,,4\r\nNA,?,x\r\n", 0, 2, ",", True))
    # a BOM before a long blank run that ends at and around a segment boundary
    for n in (61, 62, 63, 64, 130):
        for delta in (-1, 0, 1, 2, 3):
            c.append(("bom_blanks%d_%+d_label0" % (n, delta), bom_blanks(n, delta), 0, -1, ",", None))
            c.append(("bom_blanks%d_%+d_plain" % (n, delta), bom_blanks(n, delta), -1, -1, ",", None))
            c.append(("bom_blanks%d_%+d_tab" % (n, delta), bom_blanks(n, delta, "\t"), -1, -1, "\t", None))
    return c


def table():
    """What the reference does with text in special columns, one row per rule:
    [(name, text, label_column, weight_column, fast)]"""
    return [
        ("clean", "1,2.5,3\n0,7,4\n", 0, -1, True),
        ("header_label0", "label,f0,f1\n1,2.5,3\n0,,4\n", 0, -1, True),
        ("empty_label", "1,2,3\n,5,6\n", 0, -1, True),
        ("nan_value", "1,2,3\n0,nan,6\n", 0, -1, True),
        ("nan_label", "1,2,3\nnan,4,6\n", 0, -1, True),
        ("na_label", "NA,2,3\n?,4,6\n3.5kg,1,2\n", 0, -1, True),
        ("inf_label", "-inf,2,3\nInfinity,4,6\ninfo,1,2\n", 0, -1, True),
        ("blank_separators", "1, 2.5, 3\n0, 4, 5\n", 0, -1, True),
        ("bom", BOM + "1,2\n1,2\n", 0, -1, True),
        ("bom_header", BOM + "y,f0\n1,2\n", 0, -1, True),
        ("label_last", "f0,f1,y\n1,2,3\n4,5,NA\n", 2, -1, True),
        ("label_weight", "y,w,f0\n1,2,3\n4,5,6\n", 0, 1, None),
        ("label0_weight2", "y,f0,w\n1,2,3\n4,5,\n", 0, 2, None),
        ("label0_weight2_text", "y,f0,w\n1,2,3\n4,5,NA\n,,?\n", 0, 2, True),
        ("label3_weight1", "a,w,f,y\n1,2,3,4\n4,,6,NA\n", 3, 1, True),
        ("blank_special_field", "1, ,3\n4,  ,6\n", 1, -1, True),
        ("blanks_before_label", " 1,2\n  0,3\n\t1,4\n", 0, -1, True),
        ("blanks_into_text", "1, NA,3\n4, x,6\n", 1, -1, True),
        ("weight_only", "1,w,3\n4,0.5,6\n", -1, 1, True),
    ]


def violations():
    """[(name, text, label_column, weight_column)]: the exact kernels, and the
    reference's result or error."""
    return [
        ("nan_weight_one_row", "1,2,3\n4,nan,6\n", 2, 1),
        ("nan_weight_label0", "1,5,2,3\n4,5,nan,6\n", 0, 2),
        ("neg_nan_weight", "1,2,3\n4,-NaN,6\n", 2, 1),
        ("nan_paren_weight", "1,2,3\n4,NaN(ab),6\n", 2, 1),
        ("blank_nan_weight", "1,2,3\n4, +nan,6\n", 2, 1),
        ("nan_weight_every_row", "1,nan,3\n4,-NaN(x),6\n", 2, 1),
        ("nan_weight_header", "y,nanw,f\n1,2,3\n", 2, 1),
        ("short_row", "1,2,3\n4,5\n7,8,9\n", 2, -1),
        ("short_row_weight", "1,2,3,4\n4\n7,8,9,1\n", 3, 1),
        ("empty_last_label", "1,2,\n", 2, -1),
        ("empty_last_label_rows", "1,2,3\n4,5,\n7,8,9\n", 2, -1),
        ("one_field_label0", "1,2,3\n7\n", 0, -1),
        ("header_one_field_label0", "label\n1,2\n", 0, -1),
    ]
