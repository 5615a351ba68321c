"""GPU tests of dmlc_amd_gather_rows: rows ids[0 .. n) of a CSR as a new
compact CSR, word for word against tests/gather_model.py.

Hand-built CSR goes through the C call itself, into dst buffers pre-filled with
a sentinel whose every word is compared: the tail past the counts, guard
elements past each capacity and the arrays that must stay unwritten.  The edge
shapes come from the library's own geometry (R ids per tile).  Real parses go
through DeviceParser.gather_rows / gather_rows_async and are compared with the
ORACLE's CSR, or with the model over it."""
import ctypes

import numpy as np
import pytest

import dense_model as dmod
import gather_model as gm
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
WIDTHS = [(ib, vt, lt, idb) for ib in (32, 64) for vt in ("f32", "i64") for lt in ("f32", "i64") for idb in (32, 64)]
WIDTH_IDS = ["u%d-v%s-l%s-id%d" % w for w in WIDTHS]
GUARD = 3


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def _word(t):
    return U64 if t == "i64" else U32


def random_src(rng, rows, lo, hi, *, index_bits=32, vt="f32", lt="f32", value=True, weight=False, qid=False,
               field=False, lens=None):
    """-> (side, result block): rows of lo .. hi random entries, random bit patterns everywhere.  Arrays that a
    parse would not produce are one-element dummies (non-null pointers, as DeviceParser.alloc makes them)."""
    lens = rng.integers(lo, hi + 1, size=rows) if lens is None else np.asarray(lens)
    rows = len(lens)
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    nnz = int(offset[-1])
    it = U32 if index_bits == 32 else U64

    def rnd(n, word):
        return rng.integers(1, 1 << 62, size=n, dtype=np.uint64).astype(word)

    arrays = {"offset": offset, "label": rnd(rows, _word(lt)), "index": rnd(nnz, it) if nnz else np.zeros(1, it),
              "value": rnd(nnz, _word(vt)) if value and nnz else np.zeros(1, _word(vt)),
              "field": rnd(nnz, it) if field and nnz else np.zeros(1, it),
              "weight": rnd(rows, U32) if weight else np.zeros(1, U32),
              "qid": rnd(rows, U64) if qid else np.zeros(1, U64)}
    if rows == 0:
        arrays["label"] = np.zeros(1, _word(lt))
    side = gm.side_from(arrays, {gm.INDEX: nnz, gm.VALUE: nnz if value else 0, gm.FIELD: nnz if field else 0,
                                 gm.WEIGHT: rows if weight else 0, gm.QID: rows if qid else 0})
    res = np.zeros(16, dtype=U64)
    res[gm.ROWS] = res[gm.LABEL] = rows
    res[gm.INDEX] = nnz
    res[gm.VALUE] = nnz if value else 0
    res[gm.FIELD] = nnz if field else 0
    res[gm.WEIGHT] = rows if weight else 0
    res[gm.QID] = rows if qid else 0
    return side, res


def exact_caps(src, res, ids):
    """dst capacities that hold the gather exactly"""
    rows = min(int(res[gm.ROWS]), src["cap"][gm.ROWS])
    ids = np.asarray(ids).astype(U64)
    ok = ids < rows
    off = src["offset"].astype(np.int64)
    r = ids[ok].astype(np.int64)
    e = int((off[r + 1] - off[r]).sum())
    n = len(ids)
    return {gm.ROWS: n, gm.WEIGHT: n, gm.QID: n, gm.INDEX: e, gm.VALUE: e, gm.FIELD: e}


def run_c_call(dm, src, res, ids, *, index_bits=32, vt="f32", lt="f32", id_bits=64, caps=None, flags=0):
    """One dmlc_amd_gather_rows over host arrays; compares every dst word, the result block and the status
    with the model.  Returns (result block, status)."""
    import torch
    dev = torch.device("cuda", 0)
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        {4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(dev)
    ids = np.asarray(ids).astype(U64)
    caps = dict(exact_caps(src, res, ids) if caps is None else caps)
    it = U32 if index_bits == 32 else U64
    word = {"offset": U64, "label": _word(lt), "weight": U32, "qid": U64, "field": it, "index": it, "value": _word(vt)}
    size = {"offset": caps[gm.ROWS] + 1, "label": caps[gm.ROWS], "weight": caps[gm.WEIGHT], "qid": caps[gm.QID],
            "field": caps[gm.FIELD], "index": caps[gm.INDEX], "value": caps[gm.VALUE]}
    sent = {U32: 0xA5A5A5A5, U64: 0xA5A5A5A5A5A5A5A5}
    dst = gm.side_from({k: np.full(size[k] + GUARD, sent[word[k]], dtype=word[k]) for k in gm.ARRAYS}, caps)
    d_src = {k: as_t(src[k]) for k in gm.ARRAYS}
    d_dst = {k: as_t(dst[k]) for k in gm.ARRAYS}
    d_ids = as_t(ids.astype(U32 if id_bits == 32 else U64)) if len(ids) else None
    d_res = as_t(np.asarray(res, dtype=U64))
    d_dres = torch.full((16,), 0x5555, dtype=torch.int64, device=dev)
    d_status = torch.full((4,), 0x5555, dtype=torch.int64, device=dev)
    need = dm.lib().dmlc_amd_gather_workspace_bytes(len(ids))
    d_ws = torch.full((need,), 0xCD, dtype=torch.uint8, device=dev)

    def csr_of(tensors, side):
        c = dm.Csr()
        for k in gm.ARRAYS:
            setattr(c, k, tensors[k].data_ptr())
        for slot in range(7):
            c.cap[slot] = int(side["cap"].get(slot, 0))
        return c

    p = dm.GatherParams()
    p.index_bits, p.id_bits, p.flags = index_bits, id_bits, flags
    p.value_type = {"f32": dm.F32, "i32": dm.I32, "i64": dm.I64}[vt]
    p.label_type = {"f32": dm.F32, "i32": dm.I32, "i64": dm.I64}[lt]
    s_csr, d_csr = csr_of(d_src, src), csr_of(d_dst, dst)
    rc = dm.lib().dmlc_amd_gather_rows(ctypes.byref(s_csr), d_res.data_ptr(), d_ids.data_ptr() if len(ids) else None,
                                       len(ids), ctypes.byref(p), ctypes.byref(d_csr), d_dres.data_ptr(),
                                       d_status.data_ptr(), d_ws.data_ptr(), need,
                                       torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want, wres, wstatus = gm.gather_rows(src, res, ids, dst, max_index=bool(flags & dm.FLAG_MAX_INDEX))
    status = [int(x) for x in d_status.cpu().numpy().view(U64)]
    dres = [int(x) for x in d_dres.cpu().numpy().view(U64)]
    assert status == wstatus, (status, wstatus)
    assert dres == wres, (dres, wres)
    for k in gm.ARRAYS:
        got = d_dst[k].cpu().numpy().view(word[k])
        if got.tobytes() != want[k].tobytes():
            bad = np.flatnonzero(got != want[k])
            raise AssertionError("%s: %d words differ, first at %d of %d (capacity %d): got %#x want %#x"
                                 % (k, len(bad), bad[0], len(got), size[k], int(got[bad[0]]), int(want[k][bad[0]])))
    return dres, status


# ------------------------------------------------------- hand-built CSR --
def test_n_ids_around_the_tile_size(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(1)
    src, res = random_src(rng, 300, 0, 9, value=True, weight=True, qid=True, field=True)
    for n in (0, 1, R - 1, R, R + 1, 2 * R + 1):
        ids = rng.integers(0, 300, size=n)
        dres, st = run_c_call(dm, src, res, ids)
        assert dres[gm.ROWS] == n and st == [n, 0, gm.NONE, 0], n


def test_scan_run_longer_than_one_tile(dm):
    """257 R + 3 ids over rows of 0 .. 3 entries: each thread of the scan walks two tiles."""
    R = dm.gather_geometry()
    rng = np.random.default_rng(2)
    src, res = random_src(rng, 1000, 0, 3, qid=True)
    ids = rng.integers(0, 1000, size=257 * R + 3)
    for id_bits in (32, 64):
        dres, st = run_c_call(dm, src, res, ids, id_bits=id_bits)
        assert st[0] == len(ids) and dres[8] == 0


def test_all_rows_empty(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(3)
    src, res = random_src(rng, 3 * R, 0, 0)
    dres, st = run_c_call(dm, src, res, rng.integers(0, 3 * R, size=2 * R + 5))
    assert dres[gm.INDEX] == 0 and st[0] == 2 * R + 5


def test_one_long_row_among_empty_rows(dm):
    rng = np.random.default_rng(4)
    lens = np.zeros(400, dtype=np.int64)
    lens[77] = 3 * 256 * 16 + 1
    for index_bits, vt in ((32, "f32"), (64, "i64")):
        src, res = random_src(rng, 400, 0, 0, lens=lens, index_bits=index_bits, vt=vt)
        ids = (np.arange(300) * 7) % 400
        ids[ids == 77] = 78
        ids[[140, 290]] = 77  # twice
        dres, _ = run_c_call(dm, src, res, ids, index_bits=index_bits, vt=vt)
        assert dres[gm.INDEX] == 2 * (3 * 256 * 16 + 1)


def test_odd_row_lengths(dm):
    """Rows of 1, 3, 5, 7 entries: source and destination runs start off 16-byte boundaries."""
    R = dm.gather_geometry()
    rng = np.random.default_rng(5)
    lens = 1 + 2 * (np.arange(500) % 4)
    for index_bits, vt in ((32, "f32"), (32, "i64"), (64, "f32")):
        src, res = random_src(rng, 500, 0, 0, lens=lens, index_bits=index_bits, vt=vt, weight=True, field=True)
        run_c_call(dm, src, res, rng.integers(0, 500, size=R + 40), index_bits=index_bits, vt=vt)


def test_id_orders(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(6)
    rows = 2 * R + 9
    src, res = random_src(rng, rows, 0, 6, weight=True, qid=True)
    ident = np.arange(rows)
    dres, _ = run_c_call(dm, src, res, ident)
    assert dres[:8] == [int(x) for x in res[:8]]
    run_c_call(dm, src, res, ident[::-1])
    run_c_call(dm, src, res, rng.permutation(rows))
    run_c_call(dm, src, res, np.where(np.arange(R + 3) % 3, 5, np.arange(R + 3)))  # one id again and again
    run_c_call(dm, src, res, ident[::3])


def test_bad_ids(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(7)
    src, res = random_src(rng, 300, 0, 5, weight=True, qid=True, field=True)
    ids = rng.integers(0, 300, size=R + 20).astype(U64)
    ids[[3, 200]] = 300
    ids[R + 1] = 301
    for id_bits in (32, 64):
        _, st = run_c_call(dm, src, res, ids, id_bits=id_bits)
        assert st[1] == 3 and st[2] == 3
    ids[2] = (1 << 32) + 1  # not wrapped to row 1
    _, st = run_c_call(dm, src, res, ids, id_bits=64)
    assert st[1] == 4 and st[2] == 2
    dres, st = run_c_call(dm, src, res, 300 + np.arange(R + 1))
    assert st[1] == R + 1 and st[2] == 0 and dres[gm.INDEX] == 0


def test_arrays_that_are_not_there(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(8)
    for kw in (dict(value=False, qid=True), dict(), dict(weight=True, field=True)):
        src, res = random_src(rng, 300, 0, 5, **kw)
        dres, _ = run_c_call(dm, src, res, rng.integers(0, 300, size=R + 7))
        assert (dres[gm.VALUE] != 0) == kw.get("value", True) and (dres[gm.FIELD] != 0) == kw.get("field", False)
        assert (dres[gm.WEIGHT] != 0) == kw.get("weight", False) and (dres[gm.QID] != 0) == kw.get("qid", False)
    # counts that are not the row count: the arrays are not copied although their pointers are there
    src, res = random_src(rng, 300, 0, 5, weight=True, qid=True)
    res[gm.WEIGHT] = 299
    res[gm.LABEL] = 0
    dres, _ = run_c_call(dm, src, res, rng.integers(0, 300, size=R + 7))
    assert dres[gm.WEIGHT] == 0 and dres[gm.LABEL] == 0 and dres[gm.QID] == R + 7


@pytest.mark.parametrize("index_bits,vt,lt,id_bits", WIDTHS, ids=WIDTH_IDS)
def test_every_width_combination(dm, index_bits, vt, lt, id_bits):
    R = dm.gather_geometry()
    rng = np.random.default_rng(index_bits + id_bits + len(vt + lt))
    src, res = random_src(rng, 2 * R + 9, 0, 7, index_bits=index_bits, vt=vt, lt=lt, weight=True, qid=True, field=True)
    ids = rng.integers(0, 2 * R + 11, size=2 * R + 1)  # (a bad id or two)
    run_c_call(dm, src, res, ids, index_bits=index_bits, vt=vt, lt=lt, id_bits=id_bits)


def test_i32_values_and_labels(dm):
    rng = np.random.default_rng(9)
    src, res = random_src(rng, 100, 0, 7)
    run_c_call(dm, src, res, rng.permutation(100), vt="i32", lt="i32")


@pytest.mark.parametrize("slot", [gm.ROWS, gm.INDEX, gm.VALUE, gm.FIELD, gm.WEIGHT, gm.QID],
                         ids=["rows", "index", "value", "field", "weight", "qid"])
def test_each_dst_capacity_one_short(dm, slot):
    R = dm.gather_geometry()
    rng = np.random.default_rng(10 + slot)
    src, res = random_src(rng, 300, 1, 5, weight=True, qid=True, field=True)
    ids = rng.integers(0, 300, size=R + 30)
    caps = exact_caps(src, res, ids)
    total = caps[gm.INDEX]
    caps[slot] -= 1
    dres, st = run_c_call(dm, src, res, ids, caps=caps)
    # exact counts, the error word names the last position, the flag is up
    assert dres[gm.ROWS] == R + 30 and dres[gm.INDEX] == total
    assert dres[8] == ((R + 29) << 16) | gm.ERR_CAPACITY and st[3] == gm.FLAG_CAPACITY
    assert st[0] == (R + 29 if slot == gm.ROWS else R + 30)


def test_dst_capacity_far_short(dm):
    R = dm.gather_geometry()
    rng = np.random.default_rng(20)
    src, res = random_src(rng, 300, 1, 5)
    ids = rng.integers(0, 300, size=2 * R + 30)
    caps = exact_caps(src, res, ids)
    caps[gm.INDEX] //= 3  # overflows in the first tile; every later tile writes no index
    dres, st = run_c_call(dm, src, res, ids, caps=caps)
    assert dres[8] & 0xFFFF == gm.ERR_CAPACITY and 0 < dres[8] >> 16 < R
    caps = exact_caps(src, res, ids)
    caps[gm.ROWS] = 0
    dres, st = run_c_call(dm, src, res, ids, caps=caps)
    assert dres[8] == gm.ERR_CAPACITY and st[0] == 0


def test_source_errors(dm):
    rng = np.random.default_rng(30)
    src, res = random_src(rng, 50, 0, 5, field=True)
    ids = rng.integers(0, 50, size=40)
    caps = exact_caps(src, res, ids)
    bad = res.copy()
    bad[8] = (123 << 16) | 3  # a failed parse: its error is handed on, nothing is written
    dres, st = run_c_call(dm, src, bad, ids, caps=caps)
    assert st == [0, 0, gm.NONE, gm.FLAG_ERROR] and dres[8] == (123 << 16) | 3 and dres[:8] == [0] * 8
    bad = res.copy()
    bad[gm.VALUE] -= 1  # a value count that fits no RowBlock
    dres, st = run_c_call(dm, src, bad, ids, caps=caps)
    assert st == [0, 0, gm.NONE, gm.FLAG_COUNT] and dres[8] == gm.ERR_ARG
    bad = res.copy()
    bad[gm.FIELD] += 1
    bad[8] = 77 << 16 | 1
    dres, st = run_c_call(dm, src, bad, ids, caps=caps)
    assert st[3] == gm.FLAG_ERROR | gm.FLAG_COUNT and dres[8] == 77 << 16 | 1


def test_source_capacity_below_the_offsets(dm):
    """cap[INDEX] below the last offsets: clamped, flagged, and the arrays' tail past it never reaches dst."""
    rng = np.random.default_rng(31)
    src, res = random_src(rng, 400, 1, 5, field=True)
    cap = int(src["offset"][250]) - 2
    for k in ("index", "value", "field"):
        src[k][cap:] = 0xBADBAD
    src["cap"][gm.INDEX] = cap
    ids = np.arange(400)[::-1]
    caps = {gm.ROWS: 400, gm.WEIGHT: 0, gm.QID: 0, gm.INDEX: int(res[gm.INDEX]), gm.VALUE: int(res[gm.INDEX]),
            gm.FIELD: int(res[gm.INDEX])}
    dres, st = run_c_call(dm, src, res, ids, caps=caps)
    assert st[3] == gm.FLAG_OFFSET_CAP and dres[gm.INDEX] == cap
    # a row capacity below the row count: ids at or past it are bad
    src, res = random_src(rng, 300, 0, 5)
    src["cap"][gm.ROWS] = 200
    _, st = run_c_call(dm, src, res, np.arange(300))
    assert st[1] == 100 and st[2] == 200


def test_max_index_flag(dm):
    rng = np.random.default_rng(32)
    for index_bits in (32, 64):
        src, res = random_src(rng, 300, 0, 5, index_bits=index_bits, field=True)
        ids = rng.integers(0, 300, size=100)
        dres, _ = run_c_call(dm, src, res, ids, index_bits=index_bits, flags=dm.FLAG_MAX_INDEX)
        assert dres[10] > 0 and dres[11] > 0
        dres, _ = run_c_call(dm, src, res, ids, index_bits=index_bits)
        assert dres[10] == 0 and dres[11] == 0
    src, res = random_src(rng, 300, 0, 5)
    dres, _ = run_c_call(dm, src, res, [], flags=dm.FLAG_MAX_INDEX)
    assert dres[10] == 0 and dres[11] == 0


# ---------------------------------------------------- after a real parse --
def _with_qid(text, per_query=7):
    lines = text.split(b"\n")
    out = []
    for i, ln in enumerate(lines):
        if ln:
            label, rest = ln.split(b" ", 1)
            ln = label + b" qid:%d " % (i // per_query + 1) + rest
        out.append(ln)
    return b"\n".join(out)


def _parse_cases():
    lib_text = _with_qid(synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes())
    csv_text = synth.rows(synth.CSV, 200, 16, seed=9)[0].tobytes()
    fm_text = synth.rows(synth.LIBFM, 250, 8, seed=9)[0].tobytes()
    return [("libsvm", lib_text, {}), ("csv", csv_text, {"label_column": 0}), ("libfm", fm_text, {})]


_KEYS = ("offset", "label", "weight", "qid", "field", "index", "value")
_SLOT = {"label": gm.LABEL, "weight": gm.WEIGHT, "qid": gm.QID, "field": gm.FIELD, "index": gm.INDEX,
         "value": gm.VALUE}


@pytest.fixture(scope="module", params=range(3), ids=["libsvm-qid", "csv-label", "libfm"])
def parsed(request, dm):
    """(parser, device batch, the oracle's CSR as a model side + result block), parsed once per format"""
    import torch
    fmt, data, kw = _parse_cases()[request.param]
    o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt], **kw)
    assert o["status"] == 0
    p = dm.DeviceParser(fmt, flags=dm.FLAG_MAX_INDEX, **kw)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0
    it = U32
    typed = {"offset": np.asarray(o["offset"]).astype(U64), "label": np.asarray(o["label"]).astype(np.float32),
             "weight": np.asarray(o["weight"]).astype(np.float32), "qid": np.asarray(o["qid"]).astype(U64),
             "field": np.asarray(o.get("field", np.zeros(0))).astype(it), "index": np.asarray(o["index"]).astype(it),
             "value": np.asarray(o["value"]).astype(np.float32)}
    rows = len(typed["offset"]) - 1
    if fmt == "libsvm":
        assert len(typed["qid"]) == rows  # the case is about qids
    if fmt == "libfm":
        assert len(typed["field"]) == len(typed["index"]) > 0
    side = gm.side_from({k: gm.bits(v) if len(v) else None for k, v in typed.items()})
    res = np.zeros(16, dtype=U64)
    res[gm.ROWS] = rows
    for k, slot in _SLOT.items():
        res[slot] = len(typed[k])
    assert [int(x) for x in res[:8]] == [int(x) for x in out["counts"][:8]]
    return p, out, side, res, text, cs


def _host_words(dm, batch):
    h = dm.to_host(batch)
    return {k: gm.bits(np.asarray(h[k])) for k in _KEYS}


def _model_words(side, res, ids):
    """the model's gathered CSR over the oracle's, exactly sized: name -> words"""
    caps = exact_caps(side, res, ids)
    it = U32
    word = {"offset": U64, "label": U32, "weight": U32, "qid": U64, "field": it, "index": it, "value": U32}
    size = {"offset": caps[gm.ROWS] + 1, "label": caps[gm.ROWS], "weight": caps[gm.WEIGHT], "qid": caps[gm.QID],
            "field": caps[gm.FIELD], "index": caps[gm.INDEX], "value": caps[gm.VALUE]}
    dst = gm.side_from({k: np.zeros(size[k], dtype=word[k]) for k in gm.ARRAYS}, caps)
    want, wres, wstatus = gm.gather_rows(side, res, ids, dst, max_index=True)
    # what a host copy shows: each array up to its count
    n = {"offset": wres[gm.ROWS] + 1, **{k: wres[s] for k, s in _SLOT.items()}}
    return {k: want[k][:n[k]] for k in _KEYS}, wres, wstatus


def _assert_same(got, want):
    for k in _KEYS:
        assert got[k].tobytes() == want[k].tobytes(), k


def test_identity_gather_equals_the_oracle(dm, parsed):
    import torch
    p, out, side, res, _, _ = parsed
    rows = int(res[gm.ROWS])
    g = p.gather_rows(out, torch.arange(rows, device="cuda"))
    assert g["error"] == 0 and g["counts"][:8] == out["counts"][:8]
    assert [int(x) for x in g["gather_status"]] == [rows, 0, gm.NONE, 0]
    assert g["max_index"] == out["max_index"] and g["max_field"] == out["max_field"]
    got = _host_words(dm, g)
    for k in _KEYS:
        want = side[k] if side[k] is not None else np.zeros(0, got[k].dtype)
        assert got[k].tobytes() == want.tobytes(), k


def test_permuted_gather_equals_the_model_over_the_oracle(dm, parsed):
    import torch
    p, out, side, res, _, _ = parsed
    rows = int(res[gm.ROWS])
    perm = np.random.default_rng(41).permutation(rows)
    for ids in (torch.from_numpy(perm).cuda(), torch.from_numpy(perm[::2].astype(np.int32)).cuda()):
        g = p.gather_rows(out, ids)
        want, wres, wstatus = _model_words(side, res, ids.cpu().numpy())
        assert g["counts"] == wres[:8] and g["error"] == 0 and [int(x) for x in g["gather_status"]] == wstatus
        assert g["max_index"] == wres[10] and g["max_field"] == wres[11]
        _assert_same(_host_words(dm, g), want)
    g, perm = p.shuffle(out, generator=torch.Generator(device="cuda").manual_seed(5))
    assert sorted(perm.cpu().tolist()) == list(range(rows))
    _assert_same(_host_words(dm, g), _model_words(side, res, perm.cpu().numpy())[0])


def test_gather_of_a_gather_is_the_gather_of_the_composition(dm, parsed):
    import torch
    p, out, side, res, _, _ = parsed
    rows = int(res[gm.ROWS])
    rng = np.random.default_rng(42)
    a = rng.integers(0, rows, size=rows + 13)  # (ids repeat)
    b = rng.permutation(len(a))[:rows // 2]
    two = p.gather_rows(p.gather_rows(out, torch.from_numpy(a).cuda()), torch.from_numpy(b).cuda())
    one = p.gather_rows(out, torch.from_numpy(a[b]).cuda())
    assert two["counts"] == one["counts"] and two["error"] == one["error"] == 0
    _assert_same(_host_words(dm, two), _host_words(dm, one))
    _assert_same(_host_words(dm, one), _model_words(side, res, a[b])[0])


def test_parse_gather_to_dense_on_one_stream_without_a_sync(dm, parsed):
    """parse -> gather_rows_async(perm) -> to_dense_async queued back to back; the dense batch must be the dense
    model over the model's gathered CSR of the oracle's parse."""
    import torch
    p, out, side, res, text, cs = parsed
    rows, nnz = int(res[gm.ROWS]), int(res[gm.INDEX])
    perm = np.random.default_rng(43).permutation(rows)[: rows - 5]
    d_perm = torch.from_numpy(perm).cuda()
    ncol = int(out["max_index"]) + 1
    bound = rows + 50  # upper-bound buffers: every count is read on the device
    ub = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    dst = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    r1 = torch.zeros(16, dtype=torch.int64, device="cuda")
    dense = torch.full((bound, ncol), -7.0, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        p.parse_into(text, cs, ub, r1, stream=stream)
        _, r2, gst = p.gather_rows_async(ub, r1, d_perm, dst=dst, stream=stream)
        dst_status = p.to_dense_async(dst, r2, dense, ncol=ncol, fill_bits=0x7FC01234, stream=stream)
    stream.synchronize()
    want, wres, wstatus = _model_words(side, res, perm)
    assert [int(x) for x in r2.cpu().numpy().view(U64)[:12]] == wres[:12]
    assert [int(x) for x in gst.cpu().numpy().view(U64)] == wstatus
    n = len(perm)
    buf = np.full(n * ncol, 0xA5A5A5A5, dtype=U32)
    wdense, wdstatus = dmod.to_dense(want["offset"], want["index"], want["value"].view(np.float32), buf,
                                     value_dtype=np.float32, counts=(n, wres[gm.INDEX], wres[gm.VALUE]), ncol=ncol,
                                     fill_bits=0x7FC01234)
    assert [int(x) for x in dst_status.cpu().numpy().view(U64)] == wdstatus
    got = dense.cpu().numpy()
    assert got[:n].tobytes() == wdense.tobytes()
    assert (got[n:] == -7.0).all()
