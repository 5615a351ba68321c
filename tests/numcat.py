"""TEST INFRASTRUCTURE ONLY -- a deterministic catalogue of number strings at
the numeric edges of the four decoders, and an independent model of ParseFloat.

Decoders (dmlc-core_amd/csrc): decode.h parse_float / parse_uint / c_strtoll
read byte by byte; fast_common.h wfloat32m / wuint32m and csv_fast.h wint64m
read a 16-byte window and decline (*ok = false) what does not fit their form.
Every entry is tagged with the form that must decode it:

  expect "window"  the integer part has at most 8 digits, no exponent follows
                   the number, and the number (sign, digits, '.', digits) ends
                   before window byte 15, i.e. is at most 15 bytes long; for
                   wint64m additionally 1-8 digits and no leading '0' followed
                   by a digit; for wuint32m no '-'
  expect "byte"    everything else, and every string with a byte outside the
                   digit characters 0-9 + - . e E (inf / nan / suffixes /
                   0x...): the kernels never take the window's word for those

Classes (cls): frac_exhaustive, midpoint, dotpos, intpart, exponent,
degenerate, boundary, letters (kind "float"); boundary (kind "index"); ints
(kind "int").  tests/test_numcat.py pins the tags to the decoders themselves
(tests/emu/numcat_check.cpp), the oracle to the recorded reference
(tests/golden/numcat.npz) and to model_float(); tests/test_gpu_numbers.py puts
the strings into every role of every format on the device.

numpy and Python integers only.
"""
from fractions import Fraction

import numpy as np

DIGITCHARS = frozenset("0123456789+-.eE")
HEADS = ("", "0", "-7")  # frac_exhaustive: '.' at window byte 0, 1 and 2


# ------------------------------------------------------------------ tags --
def in_grammar(s):
    """Only digit characters (strtonum.h:70-72): the single-pass number grammar."""
    return len(s) > 0 and all(c in DIGITCHARS for c in s)


def _digits_from(s, a, cap=16):
    """End of the digit run of s starting at a, looking at window bytes < cap."""
    p = a
    while p < len(s) and p < cap and s[p].isdigit():
        p += 1
    return p


def expect_float(s):
    """wfloat32m's *ok on s followed by a blank, as the rule above states it."""
    if not in_grammar(s):
        return "byte"
    sg = 1 if s[0] in "+-" else 0
    p = _digits_from(s, sg)
    if p >= 16 or p - sg > 8:
        return "byte"
    pe = p
    if p < len(s) and s[p] == ".":
        pe = _digits_from(s, p + 1)
        if pe >= 16:
            return "byte"
    if pe < len(s) and s[pe] in "eE":
        return "byte"
    return "window"


def expect_index(s):
    """wuint32m's *ok and sign on s followed by a ':'."""
    if not in_grammar(s) or s[0] == "-":
        return "byte"
    sg = 1 if s[0] == "+" else 0
    return "window" if _digits_from(s, sg, 12) - sg <= 8 else "byte"


def expect_int(s):
    """wint64m's *ok on s followed by a delimiter."""
    if not s or any(c not in "0123456789+-" for c in s):
        return "byte"
    sg = 1 if s[0] in "+-" else 0
    n = _digits_from(s, sg) - sg
    if n < 1 or n > 8 or (s[sg] == "0" and n > 1):
        return "byte"
    return "window"


EXPECT = {"float": expect_float, "index": expect_index, "int": expect_int}


# ----------------------------------------------------------------- classes --
def frac_exhaustive():
    """Every fraction of 1-5 digits (111 110) under each of HEADS, as a list
    of (head, array of str).  All are tagged window."""
    fr = np.concatenate([np.char.zfill(np.arange(10 ** fl).astype(str), fl) for fl in range(1, 6)])
    return [(h, np.char.add(h + ".", fr)) for h in HEADS]


def _midpoint_digits(rng, fl, k, n, dist=None):
    """D and D + 1 with D = floor(j / 2^(25+k) * 10^fl) for n odd j in
    [2^24, 2^25): the decimals of fl digits on either side of the f32
    rounding midpoint j / 2^(25+k) of binade k (values in [2^-(k+1), 2^-k),
    where floats are the even multiples of 2^-(25+k) and the odd multiples lie
    halfway between two of them).  dist: a list that receives each string's
    distance from its midpoint relative to the midpoint, in units of 2^-64."""
    js = (rng.integers(1 << 23, 1 << 24, size=n, dtype=np.int64) * 2 + 1).tolist()
    p10, sh = 10 ** fl, 25 + k
    out = []
    for j in js:
        d = (j * p10) >> sh
        e = d + 1 if d + 1 < p10 else d - 1  # (d - 1 never: the midpoint is below 1 - 2^-25)
        out += ["%0*d" % (fl, d), "%0*d" % (fl, e)]
        if dist is not None:
            dist += [(abs((x << sh) - j * p10) << 64) // (j * p10) for x in (d, e)]
    return out


def midpoint(per=500, dist=None):
    """fl 7..14 x binade 0..7 x `per` midpoints x 2 sides: '.' + fl digits."""
    rng = np.random.default_rng(26)
    out = []
    for fl in range(7, 15):
        for k in range(8):
            out += ["." + d for d in _midpoint_digits(rng, fl, k, per, dist)]
    return out


COMPACT_MIDPOINTS = 6000


def compact_midpoints():
    """The COMPACT_MIDPOINTS strings of the midpoint class that lie closest to
    their midpoint (relative distance; the closest are within an f64 ulp of
    it, where a quotient wrong in its last bit rounds to the other float), in
    catalogue order."""
    dist = []
    mp = midpoint(dist=dist)
    keep = set(sorted(range(len(mp)), key=lambda i: (dist[i], i))[:COMPACT_MIDPOINTS])
    return [s for i, s in enumerate(mp) if i in keep]


def dotpos(per=12):
    """Midpoint neighbours behind heads of zeros, signed and not, so that the
    '.' stands at every window byte the form allows: wfloat32m takes its
    reciprocal and power of ten from table entry 16 - (byte after the '.')."""
    rng = np.random.default_rng(27)
    out = []
    for fl in range(7, 15):
        for sign in ("", "-", "+"):
            for nz in range(0, 9):
                if len(sign) + nz + 1 + fl > 15:
                    continue
                for d in _midpoint_digits(rng, fl, (fl + nz) % 8, per):
                    out.append(sign + "0" * nz + "." + d)
    return out


def intpart():
    vals = set()
    k = 0
    while 2 ** k < 10 ** 25:
        vals |= {2 ** k, 2 ** k + 1, max(2 ** k - 1, 0)}
        k += 1
    for k in range(0, 26):
        vals |= {10 ** k, 10 ** k - 1} | ({10 ** k + 1} if k < 25 else set())
    for k in range(24, 64):  # f32 ties: halfway between two floats of binade k
        vals.add(2 ** k + 2 ** (k - 24))
    for k in range(53, 64):  # u64 -> f32 through f64 would round twice
        vals |= {2 ** k + 2 ** (k - 24) + 1, 2 ** k + 2 ** (k - 24) - 1}
    strs = [str(v) for v in sorted(vals)]
    strs += ["18446744073709551615", "18446744073709551616", "1844674407370955161700123", "9" * 30,
             "00000005", "000000005", "0000000000000005"]
    out = []
    for s in strs:
        out += [s, s + ".5", s + ".000000001"]
    return out


MANTISSAS = ("1", "9.999999", "3.4028235", "3.4028236", "3.402823466", "1.17549435", "1.175494351",
             "1.1754943", "1.4", "0.7", "123456789", "0.000001")


def exponent():
    out = []
    for m in MANTISSAS:
        for x in range(-50, 46):
            if x < 0:
                out += ["%se-%d" % (m, -x), "%sE-%d" % (m, -x)]
            else:
                out += ["%se%d" % (m, x), "%sE%d" % (m, x), "%se+%d" % (m, x), "%sE+%d" % (m, x)]
        out += [m + "e-0", m + "E-0"]
    out += ["1e0000000001", "1e4294967297", "1e-4294967297", "0." + "0" * 44 + "1"]
    return out


DEGENERATE = "+ - . -. +. +.5 5. -0 -0.0 00.5 1..2 1.2.3 1-2 1+2 1e 1e+ 1e- 1.5e- e5 .e5 --1 +-1".split()
LETTERS = "inf -inf Infinity -INFINITY infinit nan NaN -nan nan(1_a) nan( nan(x 1.5f 2F".split()
RAISES = ("nan(", "nan(x")  # the reference's fatal "Invalid NAN literal": never recorded, never decoded


def boundary_floats():
    """Integer lengths 0..9 x total lengths 13..18, signed and unsigned: both
    sides of the accept / decline edge at window byte 15."""
    out = []
    for il in range(0, 10):
        for total in range(13, 19):
            for sign in ("", "-"):
                fl = total - il - 1 - len(sign)
                if fl < 0:
                    continue
                for pat in ("1234567890123456789", "9999999999999999999"):
                    out.append(sign + pat[:il] + "." + (pat + pat)[3:3 + fl])
    return out


BOUNDARY_INDEX = ["1234567", "9999999", "12345678", "99999999", "123456789", "999999999", "1234567890",
                  "4294967295", "4294967296", "4294967297", "1234567890123456", "9999999999999999",
                  "12345678901234567", "12345678901234567890", "18446744073709551615", "18446744073709551616",
                  "+1234567", "+12345678", "+123456789", "+4294967296", "0" * 19 + "5", "0000005", "00000005",
                  "000000005", "7", "0", "-5", "-0", "-12345678"]

INTS = ["1234567", "9999999", "12345678", "99999999", "123456789", "999999999", "-1234567", "-12345678",
        "-123456789", "+1234567", "+12345678", "+123456789",
        "010", "08", "00", "0x1F", "0X1f", "0x", "0xg", "-0x10", "+7", "-0", "0", "7", "-7",
        "9223372036854775807", "9223372036854775808", "-9223372036854775807", "-9223372036854775808",
        "-9223372036854775809", "+9223372036854775807",
        "2147483647", "2147483648", "2147483649", "-2147483647", "-2147483648", "-2147483649",
        "4294967295", "4294967296", "-4294967296",
        "12345678901234567890", "-12345678901234567890", "99999999999999999999999", "0777777777777777777777777",
        "0x7fffffffffffffff", "0x8000000000000000", "0xFFFFFFFFFFFFFFFFF", "00000000000000000000012"]


class Catalogue:
    """Parallel lists s / cls / kind / expect."""

    def __init__(self):
        self.s, self.cls, self.kind, self.expect = [], [], [], []

    def add(self, cls, kind, strs):
        f = EXPECT[kind]
        for x in strs:
            self.s.append(x)
            self.cls.append(cls)
            self.kind.append(kind)
            self.expect.append(f(x))

    def pick(self, kind=None, cls=None, expect=None):
        """The strings of the entries that match (cls: a name or a tuple of names)."""
        c = (cls,) if isinstance(cls, str) else cls
        return [s for s, cl, k, e in zip(self.s, self.cls, self.kind, self.expect)
                if (kind is None or k == kind) and (c is None or cl in c) and (expect is None or e == expect)]

    def counts(self, kind):
        out = {}
        for cl, k, e in zip(self.cls, self.kind, self.expect):
            if k == kind:
                w = out.setdefault(cl, [0, 0])
                w[e == "byte"] += 1
        return out


_CACHE = {}


def catalogue(compact=False):
    """Every class but frac_exhaustive (its own function: 333 330 strings).
    compact: midpoint thinned to the 6 000 strings closest to their midpoint, the set the fixture
    records and the per-role device tests use."""
    if compact in _CACHE:
        return _CACHE[compact]
    c = Catalogue()
    c.add("midpoint", "float", compact_midpoints() if compact else midpoint())
    c.add("dotpos", "float", dotpos())
    c.add("intpart", "float", intpart())
    c.add("exponent", "float", exponent())
    c.add("degenerate", "float", DEGENERATE)
    c.add("boundary", "float", boundary_floats())
    c.add("letters", "float", LETTERS)
    c.add("boundary", "index", BOUNDARY_INDEX)
    c.add("ints", "int", INTS)
    _CACHE[compact] = c
    return c


def fixture_strings():
    """The float strings tests/golden/numcat.npz records: the compact
    catalogue without the two literals the reference aborts on."""
    return [s for s in catalogue(True).pick(kind="float") if s not in RAISES]


# ------------------------------------------------------------------- model --
# ParseFloat<float> (strtonum.h:95-264) in exact arithmetic.  A float is a
# Fraction (or INF); every rounding is done here by hand, ties to even.
INF = "inf"
U64 = (1 << 64) - 1


def _rn(num, den, p, emin):
    """num / den > 0 rounded to p significant bits, exponent >= emin
    (gradual underflow): (m, e) with the result m * 2^e, m <= 2^p."""
    e = num.bit_length() - den.bit_length() - p
    for _ in range(3):  # settle 2^(p-1) <= num / den / 2^e < 2^p
        n, d = (num << -e, den) if e < 0 else (num, den << e)
        if n >= d << p:
            e += 1
        elif n < d << (p - 1):
            e -= 1
        else:
            break
    if e < emin:
        e = emin
    n, d = (num << -e, den) if e < 0 else (num, den << e)
    m, r = divmod(n, d)
    if 2 * r > d or (2 * r == d and (m & 1)):
        m += 1
    return m, e


def _pow2(m, e):
    return Fraction(m << e) if e >= 0 else Fraction(m, 1 << -e)


def rf32(x):
    """A non-negative exact value rounded to float (INF on overflow)."""
    if x is INF:
        return INF
    if x == 0:
        return Fraction(0)
    m, e = _rn(x.numerator, x.denominator, 24, -149)
    v = _pow2(m, e)
    return INF if v >= Fraction(1 << 128) else v


def rf64(num, den):
    if num == 0:
        return Fraction(0)
    return _pow2(*_rn(num, den, 53, -1074))


def f32_bits(x, negative):
    """IEEE bits of a value rf32 returned."""
    sign = 0x80000000 if negative else 0
    if x is INF:
        return sign | 0x7F800000
    if x == 0:
        return sign
    m, e = _rn(x.numerator, x.denominator, 24, -149)
    if m == 1 << 24:
        m, e = 1 << 23, e + 1
    if m < 1 << 23:
        assert e == -149
        return sign | m
    return sign | ((e + 150) << 23) + (m - (1 << 23))


K_MAX_SIG = rf32(Fraction(3402823466, 10 ** 9))      # (float)3.402823466
K_MAX_SIG_NEG = rf32(Fraction(1175494351, 10 ** 9))  # (float)1.175494351


def model_float(s):
    """(f32 bits, bytes consumed, nan_err) of ParseFloat<float> on s + NUL."""
    n = len(s)

    def at(i):
        return s[i] if i < n else "\0"

    p = 0
    while at(p) in " \t\n\r\f\v":
        p += 1
    neg = at(p) == "-"
    if at(p) in "+-":
        p += 1
    i = 0
    while i < 8 and at(p + i).lower() == "infinity"[i] and at(p + i) != "\0":
        i += 1
    if i in (3, 8):
        return f32_bits(INF, neg), p + i, False
    if s[p:p + 3].lower() == "nan":
        p += 3
        bad = False
        if at(p) == "(":
            p += 1
            while at(p).isascii() and (at(p).isalnum() or at(p) == "_"):
                p += 1
            bad = at(p) != ")"
            p += 1
        return 0x7FC00000, p, bad
    predec = 0
    while at(p).isdigit():
        predec = (predec * 10 + int(at(p))) & U64  # u64 accumulation wraps
        p += 1
    value = rf32(Fraction(predec))
    if at(p) == ".":
        p += 1
        val2, pow10, cnt = 0, 1, 0
        while at(p).isdigit():
            if cnt < 19:
                val2 = val2 * 10 + int(at(p))
                pow10 *= 10
            cnt += 1
            p += 1
        a = rf64(val2, 1)    # (double)val2
        b = rf64(pow10, 1)   # (double)pow10
        q = rf64(a.numerator * b.denominator, a.denominator * b.numerator) if a else Fraction(0)
        value = rf32(value + rf32(q))
    if at(p) in "eE":
        p += 1
        frac = at(p) == "-"
        if at(p) in "+-":
            p += 1
        expon = 0
        while at(p).isdigit():
            expon = (expon * 10 + int(at(p))) & 0xFFFFFFFF  # unsigned accumulation wraps
            p += 1
        expon = min(expon, 38)
        if expon == 38 and ((not frac and (value is INF or value > K_MAX_SIG)) or (frac and value < K_MAX_SIG_NEG)):
            value = K_MAX_SIG_NEG if frac else K_MAX_SIG
        scale = Fraction(1)
        while expon >= 8:
            scale = rf32(scale * 10 ** 8)
            expon -= 8
        while expon > 0:
            scale = rf32(scale * 10)
            expon -= 1
        if value is INF or scale is INF:  # (scale stays finite: 10^38 < 2^128)
            value = INF if scale is not INF else Fraction(0)
        else:
            value = rf32(value / scale) if frac else rf32(value * scale)
    if at(p) in "fF":
        p += 1
    return f32_bits(value, neg), p, False


def model_frac_bits(head_value, negative, digits, fl):
    """f32 bits of head '.' fraction for a small integer head: model_float's
    arithmetic on integers (the exhaustive class: 333 330 strings)."""
    q = rf64(digits, 10 ** fl)  # both operands exact in f64
    return f32_bits(rf32(head_value + rf32(q)), negative)


def py_strtoll0(s):
    """(value, bytes consumed) of strtoll(s, &e, 0): Python's own reading of
    the longest prefix int(..., 0)-style, saturated to int64."""
    p = 0
    neg = s[:1] == "-"
    if s[:1] in ("+", "-"):
        p = 1
    base, q = 10, p
    if s[p:p + 2].lower() == "0x" and s[p + 2:p + 3] and s[p + 2] in "0123456789abcdefABCDEF":
        base, q = 16, p + 2
    elif s[p:p + 1] == "0":
        base = 8
    e = q
    while e < len(s) and s[e].isascii() and s[e].isalnum() and int(s[e], 36) < base:
        e += 1
    if e == q:
        return 0, 0
    v = int(s[q:e], base)
    v = -v if neg else v
    return max(-(1 << 63), min((1 << 63) - 1, v)), e
