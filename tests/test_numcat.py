"""CPU checks of the number catalogue (tests/numcat.py).

* The oracle's ParseFloat equals the recorded genuine reference
  (tests/golden/numcat.npz) and the exact-arithmetic model numcat.model_float,
  bit for bit and in bytes consumed, on every float class of the compact
  catalogue; oracle == model on the full midpoint class and on every fraction
  of 1-5 digits under three heads (frac_exhaustive).
* The oracle's strtoll(.., 0) equals Python's own base-0 reading, saturated.
* Each entry's window / byte tag equals what the host-compiled window decoders
  report, and every value they accept equals the byte decoder's
  (tests/emu/numcat_check.cpp).
The device tests (tests/test_gpu_numbers.py) compare the kernels with the
oracle on these same strings.
"""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import numcat
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
EMU = os.path.join(HERE, "emu")
EXE = os.path.join(EMU, "_build", "numcat_check")


def load_fixture():
    z = np.load(os.path.join(HERE, "golden", "numcat.npz"))
    return z["text"].tobytes().decode("latin-1").split("\0"), z["bits"], z["used"]


def oracle_bits(strs):
    """The oracle's ParseFloat over many strings in one call: one CSV field per line."""
    o = po.parse_chunks(("\n".join(strs) + "\n").encode("latin-1"), [0, sum(len(s) + 1 for s in strs)],
                        fmt=po.CSV)
    assert o["status"] == 0 and len(o["value"]) == len(strs), (o["msg"], len(o["value"]), len(strs))
    return np.asarray(o["value"]).view(np.uint32)


def test_fixture_is_the_compact_catalogue():
    strs, bits, used = load_fixture()
    assert strs == numcat.fixture_strings()
    assert len(bits) == len(used) == len(strs)
    assert os.path.getsize(os.path.join(HERE, "golden", "numcat.npz")) <= os.path.getsize(
        os.path.join(HERE, "golden", "floats.npz"))
    cat = numcat.catalogue(True)
    assert {"midpoint", "dotpos", "intpart", "exponent", "degenerate", "boundary", "letters"} == set(cat.counts("float"))


def test_oracle_equals_fixture_equals_model():
    strs, bits, used = load_fixture()
    bad = []
    for s, b, u in zip(strs, bits.tolist(), used.tolist()):
        v, n = po.parse_float(s)
        ob = int(np.float32(v).view(np.uint32))
        mb, mn, merr = numcat.model_float(s)
        if not (ob == b == mb and n == u == mn and not merr):
            bad.append((s, hex(b), hex(ob), hex(mb), u, n, mn))
    assert bad == [], bad[:10]


def test_model_flags_the_unclosed_nan_literals():
    for s in numcat.RAISES:
        assert numcat.model_float(s)[2] is True
    assert numcat.model_float("nan(1_a)") == (0x7FC00000, 8, False)


def test_oracle_equals_model_on_every_midpoint():
    strs = numcat.catalogue(False).pick(kind="float", cls="midpoint")
    assert len(strs) == 64000
    got = oracle_bits(strs)
    exp = np.array([numcat.model_float(s)[0] for s in strs], dtype=np.uint32)
    bad = np.flatnonzero(got != exp)
    assert len(bad) == 0, [(strs[i], hex(got[i]), hex(exp[i])) for i in bad[:10]]
    # the class is what it says: each pair straddles an f32 rounding midpoint
    assert len(np.flatnonzero(got[0::2] != got[1::2])) >= 0.95 * len(strs) // 2


def test_oracle_equals_model_on_frac_exhaustive():
    groups = numcat.frac_exhaustive()
    assert [h for h, _ in groups] == list(numcat.HEADS) and all(len(a) == 111110 for _, a in groups)
    plain = []  # model: f32 bits of the fraction alone and behind "-7"
    minus7 = []
    for fl in range(1, 6):
        for d in range(10 ** fl):
            plain.append(numcat.model_frac_bits(0, False, d, fl))
            minus7.append(numcat.model_frac_bits(7, True, d, fl))
    exp = {"": plain, "0": plain, "-7": minus7}
    for head, arr in groups:
        got = oracle_bits(arr.tolist())
        bad = np.flatnonzero(got != np.array(exp[head], dtype=np.uint32))
        assert len(bad) == 0, [(arr[i], hex(got[i]), hex(exp[head][i])) for i in bad[:10]]
    for s in (".5", "0.00001", "-7.99999", "-7.1", ".33333"):  # the integer model is model_float
        head = s[:s.index(".")]
        assert numcat.model_float(s)[0] == numcat.model_frac_bits(abs(int(head or 0)), head[:1] == "-",
                                                                  int(s[s.index(".") + 1:]), len(s) - s.index(".") - 1)


@pytest.mark.parametrize("kind", [po.I64, po.I32])
def test_oracle_strtoll_equals_python(kind):
    strs = numcat.catalogue(True).pick(kind="int")
    data = ("\n".join(strs) + "\n").encode()
    o = po.parse_chunks(data, [0, len(data)], fmt=po.CSV, value_kind=kind)
    assert o["status"] == 0 and len(o["value"]) == len(strs)
    exp = [numcat.py_strtoll0(s)[0] for s in strs]
    if kind == po.I32:
        exp = [((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31) for v in exp]  # (int32_t) of the int64 result
    assert np.asarray(o["value"]).tolist() == exp, [(s, a, b) for s, a, b in zip(strs, o["value"].tolist(), exp) if a != b]
    sat = [s for s in strs if abs(numcat.py_strtoll0(s)[0]) >= (1 << 63) - 1]
    assert len(sat) >= 8  # saturation on both sides is in the list


def test_catalogue_cannot_go_hollow():
    cat = numcat.catalogue(True)
    exp = [e for k, e in zip(cat.kind, cat.expect) if k == "float"]
    nw, nb = exp.count("window"), exp.count("byte")
    # of the compact catalogue (the full one holds 64 000 midpoints, all window by construction)
    assert 3 * nw >= len(exp) and 3 * nb >= len(exp), (nw, nb)
    full = numcat.catalogue(False)
    assert set(full.pick(kind="float", cls=("midpoint", "dotpos"), expect="byte")) == set()
    for _, arr in numcat.frac_exhaustive():
        assert all(numcat.expect_float(s) == "window" for s in arr.tolist())
    for kind in ("index", "int"):
        e = [x for k, x in zip(cat.kind, cat.expect) if k == kind]
        assert e.count("window") >= 5 and e.count("byte") >= 5, kind


def test_catalogue_is_deterministic():
    a = numcat.catalogue(False)
    numcat._CACHE.clear()
    b = numcat.catalogue(False)
    assert a.s == b.s and a.expect == b.expect


@pytest.fixture(scope="module")
def emu_report(tmp_path_factory):
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_numcat"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "numcat.mk"])
    cat = numcat.catalogue(False)
    code = {"float": "f", "index": "i", "int": "n"}
    lines = ["%s %s %s" % (code[k], e[0], s) for s, k, e in zip(cat.s, cat.kind, cat.expect)]
    for _, arr in numcat.frac_exhaustive():
        lines += ["f w " + s for s in arr.tolist()]
    path = tmp_path_factory.mktemp("numcat") / "entries.txt"
    path.write_text("\n".join(lines) + "\n", encoding="latin-1")
    r = subprocess.run([EXE, str(path)], capture_output=True, timeout=120)
    return r.returncode, r.stdout.decode(), len(lines), cat


def test_tags_and_values_through_the_window_decoders(emu_report):
    rc, out, nlines, cat = emu_report
    m = re.search(r"float (\d+) window (\d+), index (\d+) window (\d+), int (\d+) window (\d+), "
                  r"tag mismatches (\d+), mismatches (\d+)", out)
    assert m, out[-2000:]
    nf, wf, ni, wi, nn, wn, tagbad, bad = map(int, m.groups())
    assert rc == 0 and tagbad == 0 and bad == 0, out[-4000:]
    assert nf + ni + nn == nlines
    fe = [e for k, e in zip(cat.kind, cat.expect) if k == "float"]
    assert wf == fe.count("window") + 3 * 111110  # every accepted one is tagged so, and the other way round
    assert wi == [e for k, e in zip(cat.kind, cat.expect) if k == "index"].count("window")
    assert wn == [e for k, e in zip(cat.kind, cat.expect) if k == "int"].count("window")
