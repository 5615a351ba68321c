"""CPU checks of the row gather (dmlc_amd_gather_rows).

tests/emu/gather_check.cpp (ASan + UBSan, built by tests/emu/gather.mk) runs
the three device tile bodies of gather_core.h with 256 host threads per tile,
for every index / value / label / id width, over n_ids in {0, 1, R-1, R, R+1,
2R+1} (R ids per tile), 257R+3 ids (the scan's per-thread run of 2 tiles),
empty rows, one 12289-entry row among empty ones, odd row lengths, every id
order, bad ids (also 2^32 + 1), absent arrays, every dst capacity one short and
every status flag, against a sequential loop in the program; whole buffers, the
result block and the status words must be equal.

The numpy model the GPU tests compare with (tests/gather_model.py) is pinned
here to three hand-written cases."""
import fcntl
import os
import re
import subprocess

import numpy as np
import pytest

import gather_model as gm

EMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "emu")
EXE = os.path.join(EMU, "_build", "gather_check")
WIDTHS = ["%s/%s/%s/%s" % (i, v, lb, d) for d in ("id32", "id64") for lb in ("l4", "l8") for v in ("v4", "v8")
          for i in ("u32", "u64")]


@pytest.fixture(scope="module")
def report():
    os.makedirs(os.path.join(EMU, "_build"), exist_ok=True)
    with open(os.path.join(EMU, "_build", ".lock_gather"), "w") as lk:  # one make among parallel workers
        fcntl.flock(lk, fcntl.LOCK_EX)
        subprocess.check_call(["make", "-s", "-C", EMU, "-f", "gather.mk"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=0:exitcode=77")
    r = subprocess.run([EXE], capture_output=True, env=env)
    out = r.stdout.decode()
    assert r.returncode == 0, out[-4000:] + r.stderr.decode()[-4000:]
    return out


def test_tile_bodies_equal_the_sequential_loop(report):
    m = re.search(r"cases (\d+), jobs (\d+), tiles (\d+), multi-tile (\d+), long-scan (\d+), bad-ids (\d+), "
                  r"overflow (\d+), mismatches (\d+)", report)
    assert m, report[-2000:]
    cases, jobs, tiles, multitile, longscan, badids, overflow, bad = map(int, m.groups())
    assert bad == 0, "\n".join(ln for ln in report.splitlines() if not ln.endswith("mismatches 0"))[-4000:]
    assert cases >= 30 and jobs >= 16 * 30 and tiles >= 1000, m.group(0)
    # each path was taken: several tiles, a scan run longer than one tile, bad ids, a capacity overflow
    assert multitile > 0 and longscan > 0 and badids > 0 and overflow > 0, m.group(0)


@pytest.mark.parametrize("widths", WIDTHS)
def test_every_width_combination_ran_every_case_group(report, widths):
    lines = [ln for ln in report.splitlines() if ("/" + widths + " ") in ln]
    groups = {ln.split("/")[0] for ln in lines}
    want = {"nids", "empty", "longrow", "odd", "order", "bad", "absent", "cap", "flag"}
    if widths in ("u32/v4/l4/id32", "u64/v8/l8/id64"):
        want.add("scanrun")
    assert groups >= want, groups
    assert all(ln.endswith("mismatches 0") for ln in lines)
    flags = {int(re.search(r"flags +(\d+)", ln).group(1)) for ln in lines if ln.startswith("flag/")}
    assert flags >= {1, 2, 4}, flags
    caps = [ln for ln in lines if ln.startswith("cap/")]
    assert len(caps) >= 5 and all(int(re.search(r"flags +(\d+)", ln).group(1)) & 8 for ln in caps)
    assert all(int(re.search(r"error ([0-9a-f]+)", ln).group(1), 16) & 0xFFFF == 16 for ln in caps)
    if widths.endswith("id64"):
        assert any(ln.startswith("bad/2^32+1") for ln in lines)


# ------------------------------------------------------------ the model --
U32, U64 = np.uint32, np.uint64
SENT = 0xA5A5A5A5


def _dst(n_rows, n_entries, names, extra=2):
    """Sentinel-filled dst buffers with `extra` elements past each capacity."""
    word = {"offset": U64, "label": U32, "weight": U32, "qid": U64, "field": U32, "index": U32, "value": U32}
    arrays = {k: np.full((n_rows + 1 if k == "offset" else n_rows if k in ("label", "weight", "qid") else n_entries)
                         + extra, SENT, dtype=word[k]) for k in names}
    cap = {gm.ROWS: n_rows, gm.WEIGHT: n_rows, gm.QID: n_rows, gm.INDEX: n_entries, gm.VALUE: n_entries,
           gm.FIELD: n_entries}
    return gm.side_from(arrays, cap)


def _f32(*v):
    return np.array(v, dtype=np.float32).view(U32)


def test_model_csv_with_a_label_column():
    # "label,f0,f1\n1,2.5,3\n0,,4\n" with label_column=0 parses to offsets [0,2,4,5],
    # labels [0,1,0] (the header row's text is 0), values [0,0,2.5,3,4]; rows 2, 0, 2 of it
    src = gm.side_from({"offset": np.array([0, 2, 4, 5], U64), "label": _f32(0, 1, 0),
                        "index": np.array([0, 1, 0, 1, 1], U32), "value": _f32(0, 0, 2.5, 3, 4)})
    res = [3, 5, 5, 0, 0, 3, 0, 0, 0]
    out, dres, status = gm.gather_rows(src, res, [2, 0, 2], _dst(3, 4, ("offset", "label", "index", "value")))
    assert list(out["offset"]) == [0, 1, 3, 4, SENT, SENT]
    assert out["label"].tolist() == _f32(0, 0, 0).tolist() + [SENT, SENT]
    assert list(out["index"]) == [1, 0, 1, 1, SENT, SENT]
    assert out["value"].tolist() == _f32(4, 0, 0, 4).tolist() + [SENT, SENT]
    assert dres[:9] == [3, 4, 4, 0, 0, 3, 0, 0, 0] and status == [3, 0, gm.NONE, 0]
    out, _, _ = gm.gather_rows(src, res, [1], _dst(1, 2, ("offset", "label", "index", "value")))
    assert out["label"][0] == _f32(1)[0] and out["value"][:2].tolist() == _f32(2.5, 3).tolist()


def test_model_libsvm_with_qid_and_no_values():
    # "1 qid:7 0 3\n0 qid:7 2\n1 qid:9 3 3 1\n": no value array, a qid per row, no weights
    src = gm.side_from({"offset": np.array([0, 2, 3, 6], U64), "label": _f32(1, 0, 1), "qid": np.array([7, 7, 9], U64),
                        "weight": np.zeros(1, U32), "index": np.array([0, 3, 2, 3, 3, 1], U32), "value": np.zeros(1, U32)})
    res = [3, 6, 0, 0, 3, 3, 0, 0, 0]
    dst = _dst(2, 4, ("offset", "label", "weight", "qid", "index", "value"))
    out, dres, status = gm.gather_rows(src, res, [2, 1], dst, max_index=True)
    assert list(out["offset"][:3]) == [0, 3, 4] and list(out["index"][:4]) == [3, 3, 1, 2]
    assert list(out["qid"][:2]) == [9, 7] and out["label"][:2].tolist() == _f32(1, 0).tolist()
    # the arrays that are not there stay as they were, and count 0
    assert (out["value"] == SENT).all() and (out["weight"] == SENT).all()
    assert dres[:9] == [2, 4, 0, 0, 2, 2, 0, 0, 0] and dres[10] == 3 and status == [2, 0, gm.NONE, 0]


def test_model_libfm_fields_duplicate_ids_and_a_bad_id():
    # "1 0:1:0.5 2:3:1.5\n0 1:2:2.5\n": fields [0,2,1], indices [1,3,2]; ids 1, 1, 5 (bad), 0
    src = gm.side_from({"offset": np.array([0, 2, 3], U64), "label": _f32(1, 0), "field": np.array([0, 2, 1], U32),
                        "index": np.array([1, 3, 2], U32), "value": _f32(0.5, 1.5, 2.5)})
    res = [2, 3, 3, 0, 0, 2, 3, 0, 0]
    dst = _dst(4, 4, ("offset", "label", "field", "index", "value"))
    out, dres, status = gm.gather_rows(src, res, [1, 1, 5, 0], dst, max_index=True)
    assert list(out["offset"][:5]) == [0, 1, 2, 2, 4]
    assert list(out["field"][:4]) == [1, 1, 0, 2] and list(out["index"][:4]) == [2, 2, 1, 3]
    assert out["value"][:4].tolist() == _f32(2.5, 2.5, 0.5, 1.5).tolist()
    assert out["label"][:4].tolist() == _f32(0, 0, 0, 1).tolist()  # the bad id's label bits are 0
    assert dres[:9] == [4, 4, 4, 0, 0, 4, 4, 0, 0] and dres[10:12] == [3, 2]
    assert status == [4, 1, 2, 0]
    # one entry short: position 3's second entry does not fit; nothing at or past the capacity is written
    dst = _dst(4, 3, ("offset", "label", "field", "index", "value"))
    out, dres, status = gm.gather_rows(src, res, [1, 1, 5, 0], dst)
    assert dres[:2] == [4, 4] and dres[8] == (3 << 16) | gm.ERR_CAPACITY and status == [4, 1, 2, gm.FLAG_CAPACITY]
    assert list(out["index"]) == [2, 2, 1, SENT, SENT] and list(out["offset"][:5]) == [0, 1, 2, 2, 4]
    # one row short: position 3 itself does not fit
    dst = _dst(3, 4, ("offset", "label", "field", "index", "value"))
    out, dres, status = gm.gather_rows(src, res, [1, 1, 5, 0], dst)
    assert dres[8] == (3 << 16) | gm.ERR_CAPACITY and status[0] == 3
    assert list(out["offset"]) == [0, 1, 2, 2, SENT, SENT] and out["label"][3] == SENT
