"""CSV text generators for the whitespace-delimiter mode of the single-pass CSV
kernel (csv_fast.h tile<.., WS>) and its integer label form.

With ' ' or '\\t' as the delimiter the number decoders skip the delimiter at a
field start, so of a maximal run of ' ' / '\\t' bytes inside a row only the
first delimiter byte after a non-blank byte separates fields; a run at a row
start separates nothing.  A run that holds a field start and reaches a line
end makes the reference read the next line's first number into this row: the
single pass declines that, so the classes that must stay on it keep at most
the structural delimiter at a line end.

clean(), runs(): inside the single-pass grammar by construction.
edge_cases(): hand-placed inputs, each with a flag saying whether it must stay
on the single pass.  violations(): outside it; parity only.
"""
import re

import numpy as np

import fuzz_text

TILE = 16384  # a single-pass tile (fast_common.h kTile)


def other(delim):
    return " " if delim == "\t" else "\t"


def _bytes(delim):
    return delim.encode("latin-1")


def _repair(line, d):
    """A ','-line turned into a delimiter-line may end in two delimiters or
    hold only delimiters (an empty last field plus a trailing delimiter, a
    line of empty fields); both leave the grammar (module docstring): keep one
    trailing delimiter, drop a delimiter-only line."""
    core = line.rstrip(d)
    if not core:
        return b""
    return core + (d if len(line) > len(core) else b"")


_INT_TOKEN = re.compile(rb"[+-]?[0-9]")


def _int_fields(line):
    """Integer values: strtoll hands back the field's start when it converts
    nothing, before the blanks it skipped, and the reference then takes one of
    those blanks as the next delimiter -- a field without an integer token
    ("e", ".", "+-2") after an empty field leaves the grammar: give it a digit."""
    f = line.split(b",")
    for i in range(1, len(f)):
        if f[i] and not f[i - 1] and not _INT_TOKEN.match(f[i]):
            f[i] = b"7" + f[i]
    return b",".join(f)


def clean(rng, nlines, maxcols=40, delim="\t", ints=False):
    """fuzz_text.uniform_csv(violate=False) bytes with ',' replaced by the
    delimiter (empty fields become delimiter runs, a leading empty field a
    leading run), line ends kept as drawn; lines that would end in more than
    one delimiter are cut back to one (_repair); ints: _int_fields."""
    raw = fuzz_text.uniform_csv(rng, nlines, maxcols, ",", violate=False)
    d = _bytes(delim)
    out, line = [], b""
    for i in range(len(raw) + 1):
        b = raw[i:i + 1]
        if b in (b"\n", b"\r", b""):
            if ints:
                line = _int_fields(line)
            out.append(_repair(line.replace(b",", d), d) + b)
            line = b""
        else:
            line += b
    return b"".join(out)


# (no hex: letters are outside the integer kernels' grammar)
_INTS = ["0", "1", "7", "42", "-5", "+7", "007", "010", "08", "123456789", "99999999999999999999",
         "-99999999999999999999", "2147483648", "-2147483649", "4294967297"]


def _field(rng, ints):
    if ints:
        return _INTS[int(rng.integers(0, len(_INTS)))] if rng.random() < 0.4 else str(int(rng.integers(-10 ** 6, 10 ** 6)))
    return "%.9g" % (rng.random() * 2 - 1) if rng.random() < 0.7 else str(int(rng.integers(0, 10 ** 5)))


def _mix(rng, n, delim):
    return "".join((delim, other(delim))[int(x)] for x in rng.integers(0, 2, size=n))


def _sep(rng, delim):
    """A run of 1-5 blanks between two fields, mixed ' ' / '\\t', with at least one delimiter."""
    n = int(rng.integers(1, 6))
    run = list(_mix(rng, n, delim))
    if delim not in run:
        run[int(rng.integers(0, n))] = delim
    return "".join(run)


def runs(rng, nlines, maxcols=30, delim="\t", ints=False):
    """Non-empty numeric fields separated by delimiter runs of 1-5 mixed
    blanks, leading runs at some row starts, and on some rows a trailing run
    that ends in its only delimiter -- no run reaches a line end with more
    than its structural delimiter, none is 63 bytes or longer."""
    o = other(delim)
    out = []
    for _ in range(nlines):
        if rng.random() < 0.03:
            out.append("")
            continue
        ncol = int(rng.integers(1, maxcols + 1))
        line = _mix(rng, int(rng.integers(1, 6)), delim) if rng.random() < 0.2 else ""
        line += _field(rng, ints)
        for _ in range(ncol - 1):
            line += _sep(rng, delim) + _field(rng, ints)
        r = rng.random()
        if r < 0.1:
            line += delim
        elif r < 0.15:
            line += o * int(rng.integers(1, 4)) + delim
        elif r < 0.2:
            line += o * int(rng.integers(1, 4))  # blanks without a delimiter: no field starts in them
        out.append(line)
    seps = ["\n"] * 12 + ["\r\n", "\r", "\n\n"]
    text = "".join(line + seps[int(rng.integers(0, len(seps)))] for line in out)
    if rng.random() < 0.3:
        text = text.rstrip("\r\n")
    return text.encode("latin-1")


def _fill_to(target, delim):
    """Rows of short fields, then the head of a row, ending in a digit at byte target - 1."""
    row = "1%s22%s333\n" % (delim, delim)
    n = max(0, (target - 12) // len(row))
    head = row * n
    rest = target - len(head)
    assert rest >= 1
    k = (rest - 1) // 4
    return head + ("123" + delim) * k + "9" * (rest - 4 * k)


def straddle(boundary, split, run, delim):
    """Text whose blank run `run` starts `split` bytes before `boundary`."""
    pre = _fill_to(boundary - split, delim)
    assert len(pre) == boundary - split
    return (pre + run + "5%s6\n7%s8\n" % (delim, delim)).encode("latin-1")


def edge_cases(delim):
    """[(name, data, chunk offsets or None for random cuts anywhere, fast, f32 only)]:
    `fast` = the input must stay on the single pass."""
    o = other(delim)
    run = o + o + delim + delim + o  # structural delimiter at run[2]
    c = []
    # a run across a 64-byte segment end and a 16 KiB tile end (before, at and
    # after its structural delimiter), and across the start of the tile's 64 B pre-halo
    for name, bnd in (("seg", 64), ("seg3", 192), ("tile", TILE), ("prehalo", TILE - 64), ("tile2", 2 * TILE)):
        for split in range(0, len(run) + 1):
            c.append(("%s_split%d" % (name, split), straddle(bnd, split, run, delim), "whole", True, False))
    # exactly 62 blanks at several alignments, the delimiter early, in the middle, last
    for at in (1, 30, 63, 64, 100):
        for pos in (0, 31, 61):
            r62 = o * pos + delim + o * (61 - pos)
            c.append(("run62_at%d_d%d" % (at, pos), (_fill_to(at, delim) + r62 + "2\n3%s4\n" % delim).encode("latin-1"),
                      "whole", True, False))
    # 64 blanks and more: either path
    for n in (64, 65, 130, 200):
        for pos in (0, n // 2, n - 1):
            rn = o * pos + delim + o * (n - 1 - pos)
            c.append(("run%d_d%d" % (n, pos), ("3%s4\n1" % delim + rn + "2\n").encode("latin-1"), "whole", False, False))
    # chunk starts inside runs and right after structural delimiters
    body = ("1%s2%s%s3%s%s%s4\n" % (delim, delim, o, o, delim, delim) * 9).encode("latin-1")
    c.append(("cuts_anywhere", body, None, False, False))
    k = body.index(_bytes(delim)) + 1
    c.append(("cut_after_structural", body, [0, k, len(body)], False, False))
    c.append(("cut_inside_run", body, [0, body.index(_bytes(o + delim + delim)) + 2, len(body)], False, False))
    # one row longer than two tiles: the segmented column count crosses tiles through the look-back
    wide = (delim + o).join(str(i % 1000) for i in range(9000)) + "\n" + "1%s2\n" % delim
    assert len(wide) > 2 * TILE + 4000
    c.append(("row_over_two_tiles", wide.encode("latin-1"), "whole", True, False))
    c.append(("crlf", ("1%s2%s%s3\r\n4%s5\r\n\r\n6%s7%s\r\n" % (delim, delim, o, delim, delim, delim)).encode("latin-1"),
              "whole", True, False))
    c.append(("header_words", ("id%sname%s%sscore\n1%s2%s3\n" % (delim, o, delim, delim, delim)).encode("latin-1"),
              "whole", True, True))
    c.append(("junk_after_blanks", ("1%s%sabc%s5\n2%s%s%sx\n" % (delim, o, delim, delim, delim, o)).encode("latin-1"),
              "whole", True, True))
    return c


def table(delim):
    """What the reference does with a whitespace delimiter, one row per rule
    (written with '\\t' as the delimiter and ' ' as the other blank; swapped
    for ' ').  [(name, text, fast)]; "text_fields" is fast for float values
    only (text is outside the integer kernels' grammar)."""
    rows = [("clean", "1\t2\t3", True), ("run_once", "1\t\t3", True), ("run_long", "1\t\t\t\t2", True),
            ("leading_run", "\t1\t2", True), ("mixed_after", "1\t 2", True), ("mixed_before", "1 \t2", True),
            ("one_trailing", "1\t2\t\n", True), ("two_trailing_phantom", "1\t2\t\t\n3\t4", False),
            ("two_trailing_chunk_end", "1\t2\t\t\n", False), ("text_fields", "a\tb", True),
            ("other_blank_no_separator", "1 2 3", True)]
    sw = {"\t": delim, " ": other(delim)}
    return [(n, "".join(sw.get(ch, ch) for ch in t), f) for n, t, f in rows]


def violations(delim):
    """Inputs outside the single-pass grammar: parity only.  [(name, data, offsets)]"""
    o = other(delim)
    d = delim
    c = [
        ("two_trailing_mid", "1%s2%s%s\n3%s4\n" % (d, d, d, d), None),
        ("two_trailing_chunk_end", "1%s2%s%s\n" % (d, d, d), None),
        ("two_trailing_at_cut", "1%s2%s%s\n3%s4\n" % (d, d, d, d), [0, 6, 10]),
        ("three_trailing_no_eol", "1%s2%s%s%s" % (d, d, d, d), None),
        ("trailing_then_other", "1%s2%s%s\n3\n" % (d, d, o), None),
        ("vt_in_run", "1%s\v%s2\n3%s4\n" % (d, d, d), None),
        ("ff_in_run", "1%s\f2\n3\f%s4\n" % (d, d), None),
        ("blank_only_row", "1%s2\n%s%s\n3%s4\n" % (d, d, o, d), None),
        ("blank_only_row_other", "1%s2\n%s%s\n3%s4\n" % (d, o, o, d), None),
        ("other_as_delimiter", "1%s2%s3\n4%s5%s6\n" % (o, o, o, d), None),
        ("other_only", "1%s2%s3\n" % (o, o), None),
        # integer values: no token after skipped delimiters (_int_fields)
        ("no_token_after_run", "1%s%se%s%s5\n%s%s.%s6\n" % (d, d, d, d, d, d, d), None),
        ("sign_after_run", "1%s%s%s-%s+%s%s-2\n" % (d, o, d, d, d, d), None),
    ]
    return [(n, t.encode("latin-1"), offs) for n, t, offs in c]


def with_delim(data, delim):
    """',' text (fuzz_text.labeled_csv, tools.synth) with the delimiter swapped in."""
    return data.replace(b",", _bytes(delim))


def doubled(data, delim, rng):
    """One delimiter of the text doubled: outside the label / weight kernels' clean form."""
    d = _bytes(delim)
    pos = [i for i in range(len(data)) if data[i:i + 1] == d]
    k = pos[int(rng.integers(0, len(pos)))]
    return data[:k] + d + data[k:]


def int_label_defect(rng, nlines, ncols, label_col, kind, delim=","):
    """labeled_csv with one defect row: 'empty' label field, or a 'one_field' row."""
    data = fuzz_text.labeled_csv(rng, nlines, ncols, label_col, delim)
    lines = data.decode("latin-1").split("\n")[:-1]
    k = int(rng.integers(0, len(lines)))
    f = lines[k].split(delim)
    if kind == "empty":
        f[min(label_col, ncols - 1)] = ""
    else:
        f = f[:1]
    lines[k] = delim.join(f)
    return ("\n".join(lines) + "\n").encode("latin-1")


def sized(gen, nbytes):
    """Call gen(nlines) with growing nlines until it returns about nbytes, then cut at a line end."""
    n = 64
    data = gen(n)
    while len(data) < nbytes + 200:
        n *= 2
        data = gen(n)
    k = data.index(b"\n", nbytes - 40) + 1
    return data[:k]
