"""CPU checks of the captured-graph tests' inputs (tests/graph_cases.py): what
tests/test_gpu_graph.py relies on is verified here with the oracle, the
emulator and the numpy models alone -- equal byte and chunk counts inside a
family, the labelled status of every member, A and B apart in every array and
count (a replay that handed back the previous replay's results cannot pass),
E past the captured capacities, and the path A, B and C take."""
import numpy as np
import pytest

import full_call as fc
import graph_cases as gc
from golden_util import diff
from oracle import pyoracle as po
from tests.emu import pyemu, pyemu_ws


def _tile():
    import dmlc_amd
    return dmlc_amd.fast_geometry()[0]


def _geom():
    import dmlc_amd as dm
    return {"csc": dm.csc_geometry()[0], "cuts": dm.make_cuts_geometry()[0], "gather": dm.gather_geometry(),
            "dense": dm.dense_geometry(), "bins": dm.bins_geometry()}


def _emu(fam, member, kw):
    m = fam["members"][member]
    ekw = {k: v for k, v in kw.items() if k != "flags"}
    if fam["fmt"] == po.CSV:
        return pyemu_ws.parse(m["data"], m["offs"], **ekw)
    return pyemu.parse(m["data"], m["offs"], fc.FMT_NAME[fam["fmt"]], **ekw)


@pytest.mark.parametrize("name", gc.FAMILIES)
def test_family_sizes_are_equal_and_three_tiles_plus_a_remainder(name):
    tile = _tile()
    fam = gc.family(name, tile)
    assert set(fam["members"]) == set("ABCDE") and fam["nchunks"] >= 3
    for m in fam["members"].values():
        assert len(m["data"]) == fam["nbytes"] == 3 * tile + gc.REM, m["name"]
        assert len(m["offs"]) == fam["nchunks"] + 1 and m["offs"][0] == 0 and m["offs"][-1] == fam["nbytes"], m["name"]
        assert all(m["data"][c - 1:c] == b"\n" for c in m["offs"][1:]), m["name"]  # cut at line starts
    A, B, C, D = (fam["members"][k] for k in "ABCD")
    assert A["offs"] != B["offs"]
    for m, line in ((C, fam["violate"]), (D, fam["error_line"])):  # the placed line, in the middle tile
        at = m["at"]
        assert tile <= at and at + len(line) < 2 * tile
        assert m["data"][at - 1:at + len(line) + 1] == b"\n" + line + b"\n", m["name"]
        assert m["data"][:at] == A["data"][:at]


@pytest.mark.parametrize("config", sorted(gc.CONFIGS))
def test_family_members_are_as_labelled(config):
    """Per parse-graph configuration: the oracle's status per member, A / B
    apart, the captured capacities, and the emulator's path and error word."""
    import dmlc_amd
    tile = _tile()
    name, kw = gc.config_kw(config)
    fam = gc.family(name, tile)
    o = {m: gc.oracle_of(fam, m, kw) for m in "ABCDE"}
    for m in "ABCE":
        assert o[m]["status"] == 0, (m, o[m]["msg"])
    assert o["D"]["status"] != 0
    code = fam["members"]["D"]["err"][0]
    assert ("sign == true" in o["D"]["msg"]) == (code == gc.ERR_NEG_INDEX), o["D"]["msg"]
    assert ("elimiter" in o["D"]["msg"]) == (code == gc.ERR_CSV_DELIM), o["D"]["msg"]
    # A and B: every array the format produces differs, and every count it produces
    ca, cb = fc.oracle_counts(o["A"]), fc.oracle_counts(o["B"])
    for s in range(7):
        assert (ca[s] == 0 and cb[s] == 0) or ca[s] != cb[s], (s, ca, cb)
    assert ca[fc.ROWS] > cb[fc.ROWS] and ca[fc.INDEX] * cb[fc.ROWS] < cb[fc.INDEX] * ca[fc.ROWS]  # fewer, longer rows
    for k in fc.ARRAYS:
        a, b = np.asarray(o["A"][k]), np.asarray(o["B"][k])
        assert (len(a) == 0 and len(b) == 0) or a.tobytes() != b.tobytes(), k
        n = min(len(a), len(b))  # (not one a prefix of the other either)
        assert n == 0 or k == "offset" and n == 1 or a[:n].tobytes() != b[:n].tobytes(), k
    caps = gc.captured_caps(o)
    for m in "ABC":
        assert all(c + gc.SLACK <= cap for c, cap in zip(fc.oracle_counts(o[m]), caps)), m
    ce = fc.oracle_counts(o["E"])
    assert ce[fc.INDEX] > caps[fc.INDEX], (ce, caps)
    exact = bool(kw.get("flags", 0) & gc.FLAG_EXACT)
    for m in "ABCD":
        h = _emu(fam, m, kw)
        nunits = fam["nchunks"] * max(kw.get("nthread", 1), 1)
        failed = bool(h["error"]) or dmlc_amd.chunk_check(h, fc.FMT_NAME[fam["fmt"]], nunits, h["counts"]) >= 0
        assert failed == (m == "D"), (m, h["error"])
        if m == "D":  # the first error by position: its code and the byte the kernels name
            ecode, epos = fam["members"]["D"]["err"]
            assert h["error"] == (epos << 16) | ecode, (h["error"] >> 16, h["error"] & 0xFFFF, epos, ecode)
            continue
        assert diff(h, o[m]) == [], (m, diff(h, o[m]))
        assert h["path"] == ("fast" if fam["members"][m]["expect"] == "stay" else "exact"), (m, h["path"])
        if exact:
            assert _emu(fam, m, dict(kw, exact=True))["path"] == "exact"


def _differ(a, b, keys=None):
    return [k for k in (keys or a) if np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes()]


def test_chain_family():
    geom = _geom()
    fam = gc.chain_family(geom)
    M = fam["members"]
    assert set(M) == {"A", "B", "D", "A2"}
    for m in M.values():
        assert len(m["data"]) == fam["nbytes"] and len(m["offs"]) == fam["nchunks"] + 1 == 4, m["name"]
        assert all(m["data"][c - 1:c] == b"\n" for c in m["offs"][1:]), m["name"]
    assert M["A"]["offs"] != M["B"]["offs"] and M["A"]["data"] != M["A2"]["data"]
    o = {m: gc.chain_oracle(fam, m) for m in M}
    assert all(o[m]["status"] == 0 for m in ("A", "B", "A2")) and o["D"]["status"] != 0 and "elimiter" in o["D"]["msg"]
    assert gc.oracle_of(fam, "A", fam["kw"])["index"].max() == gc.CHAIN_NCOL - 1
    for k in ("offset", "index"):  # A2 moves values only
        assert o["A"][k].tobytes() == o["A2"][k].tobytes()
    assert o["A"]["value"].tobytes() != o["A2"]["value"].tobytes()
    ids1, ids2 = fam["ids"][1], fam["ids"][2]
    n = fam["n_ids"]
    assert len(ids1) == len(ids2) == n > 2 * geom["gather"]
    assert len(np.unique(ids1)) == n and ids1.max() < len(o["A"]["offset"]) - 1 and ids1.max() < len(o["B"]["offset"]) - 1
    assert len(np.unique(ids2)) < n and int((ids2 == (1 << 32) + 1).sum()) == 1
    d = gc.chain_dims(fam, o)
    want = {(m, w): gc.chain_expect(o[m], 0, fam["ids"][w], d) for m, w in (("A", 1), ("B", 1), ("A", 2), ("A2", 1))}
    for w in want.values():  # sizes: more than two tiles everywhere, nothing truncated
        rows, ent = int(w["g_res"][gc.gm.ROWS]), int(w["g_res"][gc.gm.INDEX])
        assert rows == n and w["g_res"][8] == 0 and ent + 50 <= d["g_ent"] and ent > 2 * geom["csc"]
        assert int(w["cuts_status"][gc.qm.KEPT]) > 2 * geom["cuts"] and w["cuts_status"][3] == 0
        assert 0 < int(w["cuts_status"][gc.qm.N_CUTS]) <= d["cut_cap"]
        for g in ("dense", "bins"):
            cells, most = geom[g]
            assert rows > 2 * min(most, cells // min(gc.CHAIN_NCOL, cells))
        assert int(w["csc_status"][0]) == ent and w["csc_status"][3] == 0 and w["dense_status"][3] == 0
        assert w["bins_status"][3] == 0 and int(w["bins_status"][0]) == n
    assert int(want[("A", 2)]["g_status"][1]) == 1  # the bad id
    outs = ("g_offset", "g_label", "g_index", "g_value", "cut_ptr", "cut_value", "bins", "dense", "csc_col_offset",
            "csc_row", "csc_value", "csc_pos")
    keys = list(want)
    for i in range(len(keys)):
        for j in range(i + 1, len(keys)):
            same = _differ(want[keys[i]], want[keys[j]], outs)
            if {keys[i], keys[j]} == {("A", 1), ("A2", 1)}:  # only values moved: the values, the cuts and the codes differ
                assert not set(same) & {"g_value", "cut_value", "bins", "dense", "csc_value"}, same
            else:
                assert same == [], (keys[i], keys[j], same)
    # D: the error goes down the chain; cut_ptr and col_offset are zeroed (dmlc_amd.h), all else keeps its sentinel
    ecode, epos = M["D"]["err"]
    w = gc.chain_expect(None, (epos << 16) | ecode, ids1, d)
    assert w["g_status"][3] == 1 and w["cuts_status"][3] == 1 and w["bins_status"][3] == 1
    assert w["dense_status"][3] == 1 and w["csc_status"][3] == 1 and int(w["g_res"][8]) == (epos << 16) | ecode
    for k in outs:
        a = np.asarray(w[k])
        if k in ("cut_ptr", "csc_col_offset"):
            assert not a[:gc.CHAIN_NCOL + 1].any() and (a[gc.CHAIN_NCOL + 1:].view(np.uint8) == gc.SENT).all(), k
        else:
            assert (a.view(np.uint8) == gc.SENT).all(), k

