"""GPU tests of dmlc_amd_to_csc: the entries of a CSR's row window by column,
word for word against tests/csc_model.py.

Hand-built CSR goes through the C call itself.  The outputs are pre-filled with
0xA5.. and the workspace with 0xCD; every output word is compared with the
model: guard words past the capacity and arrays that must stay unwritten
included.  The edge shapes come from the library's own geometry (T entries per
tile).  Real parses go through DeviceParser.to_csc / to_csc_async and are
compared with the model over the ORACLE's CSR.  Nothing has a tolerance: every
comparison is of bit patterns."""
import ctypes

import numpy as np
import pytest

import csc_model as cm
import dense_model as dmod
import gather_model as gm
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
GUARD = 3
SENT = {U32: 0xA5A5A5A5, U64: 0xA5A5A5A5A5A5A5A5}


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def _word(vt):
    return U64 if vt == "i64" else U32


def make_csr(rng, lens, ncol_max, *, index_bits=32, vt="f32", value=True):
    """rows of the given lengths, columns below ncol_max, random value bits"""
    lens = np.asarray(lens, dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    nnz = int(offset[-1])
    it = U32 if index_bits == 32 else U64
    index = rng.integers(0, ncol_max, size=nnz, dtype=np.uint64).astype(it)
    val = rng.integers(1, 1 << 62, size=nnz, dtype=np.uint64).astype(_word(vt)) if value else None
    return offset, index, val


def run_c_call(dm, offset, index, value, *, ncol, index_bits=32, vt="f32", counts=None, row_begin=0, max_rows=None,
               cap=None, want_val=True, want_pos=True, cap_rows=None, cap_index=None, cap_value=None, error=0,
               max_entries=0, ws=None):
    """One dmlc_amd_to_csc over host arrays; compares every output word and the status with the model.
    Returns (outputs, status)."""
    import torch
    dev = torch.device("cuda", 0)
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        {4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(dev)
    it = U32 if index_bits == 32 else U64
    offset = np.asarray(offset, dtype=U64)
    index = np.asarray(index, dtype=it)
    nnz = len(index)
    rows = len(offset) - 1
    if counts is None:
        counts = (rows, nnz, nnz if value is not None else 0)
    cap_rows = rows if cap_rows is None else cap_rows
    cap_index = nnz if cap_index is None else cap_index
    if cap_value is None:
        cap_value = nnz if value is not None else 0
    vw = _word(vt)
    # the model's outputs = the device's, pre-filled
    if cap is None:
        cap = nnz
    bufs = {"col_offset": np.full(ncol + 1 + GUARD, SENT[U64], U64), "row": np.full(cap + GUARD, SENT[U32], U32),
            "value": np.full(cap + GUARD, SENT[vw], vw) if want_val else None,
            "pos": np.full(cap + GUARD, SENT[U64], U64) if want_pos else None, "cap": cap}
    d_out = {k: as_t(v) for k, v in bufs.items() if k != "cap" and v is not None}
    d_off = as_t(offset)
    d_idx = as_t(index if nnz else np.zeros(1, it))
    d_val = as_t(value if value is not None and nnz else np.zeros(1, vw))
    res = np.zeros(16, dtype=U64)
    res[dm.ROWS], res[dm.INDEX], res[dm.VALUE], res[8] = counts[0], counts[1], counts[2], error
    d_res = as_t(res)
    d_status = torch.full((4,), 0x5555, dtype=torch.int64, device=dev)
    csr = dm.Csr()
    csr.offset, csr.index = d_off.data_ptr(), d_idx.data_ptr()
    csr.value = d_val.data_ptr() if value is not None else None
    csr.cap[dm.ROWS], csr.cap[dm.INDEX], csr.cap[dm.VALUE] = cap_rows, cap_index, cap_value
    p = dm.CscParams()
    p.index_bits, p.value_type = index_bits, {"f32": dm.F32, "i32": dm.I32, "i64": dm.I64}[vt]
    p.row_begin, p.max_rows = row_begin, (1 << 64) - 1 if max_rows is None else max_rows
    p.ncol, p.max_entries = ncol, max_entries
    need = dm.lib().dmlc_amd_csc_workspace_bytes(min(max_entries, cap_index) if max_entries else cap_index, ncol,
                                                 ctypes.byref(p))
    assert need > 0
    if ws is None:
        ws = torch.full((need,), 0xCD, dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    c = dm.Csc()
    c.col_offset, c.row = d_out["col_offset"].data_ptr(), d_out["row"].data_ptr()
    c.value = d_out["value"].data_ptr() if want_val else None
    c.pos = d_out["pos"].data_ptr() if want_pos else None
    c.cap = cap
    rc = dm.lib().dmlc_amd_to_csc(ctypes.byref(csr), d_res.data_ptr(), ctypes.byref(p), ctypes.byref(c),
                                  d_status.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    want, wstatus = cm.to_csc(offset, index, value, bufs, counts=counts, ncol=ncol, error=error, cap_rows=cap_rows,
                              cap_index=cap_index, cap_value=cap_value, row_begin=row_begin, max_rows=max_rows,
                              max_entries=max_entries)
    status = [int(x) for x in d_status.cpu().numpy().view(U64)]
    print("ncol %d entries %d status %s" % (ncol, nnz, status))
    assert status == wstatus, (status, wstatus)
    got = {}
    for k, t in d_out.items():
        got[k] = t.cpu().numpy().view(bufs[k].dtype)
        if got[k].tobytes() != want[k].tobytes():
            bad = np.flatnonzero(got[k] != want[k])
            raise AssertionError("%s: %d words differ, first at %d of %d (capacity %d): got %#x want %#x"
                                 % (k, len(bad), bad[0], len(got[k]), cap, int(got[k][bad[0]]), int(want[k][bad[0]])))
    return got, status


def lens_for(rng, n, hi=9):
    """row lengths of 0 .. hi summing to exactly n"""
    lens = []
    left = n
    while left > 0:
        m = min(int(rng.integers(0, hi + 1)), left)
        lens.append(m)
        left -= m
    return lens + [0, 0]


# ------------------------------------------------------- hand-built CSR --
def test_entry_counts_around_the_tile_size(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(1)
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        off, idx, val = make_csr(rng, lens_for(rng, n), 210)
        _, st = run_c_call(dm, off, idx, val, ncol=200)
        assert st[0] + st[1] == n and st[3] == 0, n


def test_scan_run_longer_than_one_tile(dm):
    """257 T + 3 entries: each thread of the scan walks two tiles."""
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(2)
    n = 257 * T + 3
    lens = np.full(n // 37 + 1, 37)
    lens[-1] = n - 37 * (n // 37)
    off, idx, val = make_csr(rng, lens, 256)
    _, st = run_c_call(dm, off, idx, val, ncol=256)
    assert st == [n, 0, cm.NONE, 0]


@pytest.mark.parametrize("ncol,npass", [(1, 1), (2, 1), (255, 1), (256, 1), (257, 2), (65536, 2), (65537, 3),
                                        (1 << 24, 3), ((1 << 24) + 1, 4)])
def test_ncol_and_the_pass_count(dm, ncol, npass):
    T, _ = dm.csc_geometry()
    assert cm.passes(ncol) == npass
    rng = np.random.default_rng(ncol)
    off, idx, val = make_csr(rng, rng.integers(0, 9, size=T // 4 + 100), ncol + (3 if ncol > 2 else 1))
    if ncol > 300:  # the top columns are there, and entries just past them
        idx[:3] = [ncol - 1, ncol - 2, 0]
        idx[10:13] = [ncol, ncol + 1, ncol + 2]
    got, st = run_c_call(dm, off, idx, val, ncol=ncol)
    assert st[0] + st[1] == len(idx) > T and st[0] > 0 and st[1] > 0  # (more than one tile)
    if ncol > 300:
        assert got["col_offset"][ncol] - got["col_offset"][ncol - 1] >= 1


def test_every_entry_in_one_column(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(3)
    n = 2 * T + 1
    off, idx, val = make_csr(rng, lens_for(rng, n, 30), 1)
    got, st = run_c_call(dm, off, idx, val, ncol=1)
    assert st[0] == n and (got["pos"][:n] == np.arange(n)).all()
    idx[:] = 300
    got, st = run_c_call(dm, off, idx, val, ncol=65537)
    assert st[0] == n and (got["pos"][:n] == np.arange(n)).all()
    assert got["col_offset"][300] == 0 and got["col_offset"][301] == n


def test_columns_that_differ_only_in_a_high_digit(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(4)
    off, idx, val = make_csr(rng, lens_for(rng, T + 77), 3)
    idx[:] = np.array([5, 5 + 256, 5 + 65536], U32)[idx]
    got, st = run_c_call(dm, off, idx, val, ncol=70000)
    assert st[0] == T + 77 and st[1] == 0


def test_each_rows_columns_descending_and_a_cell_three_times(dm):
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 12, size=900)
    off, idx, val = make_csr(rng, lens, 300)
    for r in range(len(lens)):
        a, b = int(off[r]), int(off[r + 1])
        idx[a:b] = np.sort(idx[a:b])[::-1]
    run_c_call(dm, off, idx, val, ncol=300)
    # the same cell three times in a row, then another entry
    lens = np.full(1500, 4)
    off, idx, val = make_csr(rng, lens, 50)
    idx[1::4] = idx[0::4]
    idx[2::4] = idx[0::4]
    got, _ = run_c_call(dm, off, idx, val, ncol=50)
    co, pos = got["col_offset"][:51].astype(np.int64), got["pos"][:6000].astype(np.int64)
    assert all((np.diff(pos[co[c]:co[c + 1]]) > 0).all() for c in range(50))  # ascending position inside a column


def test_dropped_entries(dm):
    rng = np.random.default_rng(6)
    off, idx, val = make_csr(rng, rng.integers(1, 7, size=2000), 100)
    idx[7], idx[3], idx[500] = 100, 101, 0xFFFFFFFF
    _, st = run_c_call(dm, off, idx, val, ncol=100)
    assert st[1] == 3 and st[2] == 3
    # 64-bit indices: 2^32 + c must not land in column c
    off, idx, val = make_csr(rng, rng.integers(1, 7, size=2000), 100, index_bits=64)
    idx[2], idx[600], idx[9] = (1 << 32) + 5, (1 << 32) + 99, (1 << 63) + 1
    _, st = run_c_call(dm, off, idx, val, ncol=100, index_bits=64)
    assert st[1] == 3 and st[2] == 2
    # every entry dropped
    idx[:] = idx + np.uint64(100)
    _, st = run_c_call(dm, off, idx, val, ncol=100, index_bits=64)
    assert st[0] == 0 and st[1] == len(idx) and st[2] == 0


def test_empty_rows(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(7)
    lens = np.concatenate([np.zeros(100, np.int64), rng.integers(0, 5, size=2 * T // 2), np.zeros(100, np.int64)])
    off, idx, val = make_csr(rng, lens, 64)
    run_c_call(dm, off, idx, val, ncol=64)
    # 10 000 empty rows between two entries of one tile: the tile's offsets do not fit its LDS span
    lens = np.concatenate([rng.integers(1, 4, size=150), np.zeros(10000, np.int64), rng.integers(1, 4, size=150)])
    off, idx, val = make_csr(rng, lens, 64)
    assert int(off[-1]) < T
    got, _ = run_c_call(dm, off, idx, val, ncol=64)
    assert got["row"][:int(off[-1])].max() >= 10150


def test_tiles_inside_a_single_row(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(8)
    lens = np.zeros(300, dtype=np.int64)
    lens[77] = 3 * T + 5
    for ncol in (256, 257):
        off, idx, val = make_csr(rng, lens, ncol)
        got, st = run_c_call(dm, off, idx, val, ncol=ncol)
        assert st[0] == 3 * T + 5 and (got["row"][:st[0]] == 77).all()


def test_row_windows(dm):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(9)
    lens = rng.integers(0, 8, size=3 * T // 3)
    off, idx, val = make_csr(rng, lens, 303)
    rows = len(lens)
    for ncol in (300, 70000):
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, row_begin=rows // 3 + 1)  # begins inside a tile
        assert 0 < st[0] < len(idx)
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, row_begin=17, max_rows=rows // 2)  # max_rows cuts a tile
        assert 0 < st[0] < len(idx)
        assert run_c_call(dm, off, idx, val, ncol=ncol, max_rows=0)[1] == [0, 0, cm.NONE, 0]
        assert run_c_call(dm, off, idx, val, ncol=ncol, row_begin=rows)[1] == [0, 0, cm.NONE, 0]
        assert run_c_call(dm, off, idx, val, ncol=ncol, row_begin=rows + 5, max_rows=3)[1] == [0, 0, cm.NONE, 0]
    # a row capacity below the count, and the caller's own bound on the window's entries
    run_c_call(dm, off, idx, val, ncol=300, cap_rows=rows - 500)
    e = int(off[1100] - off[100])
    _, st = run_c_call(dm, off, idx, val, ncol=300, row_begin=100, max_rows=1000, max_entries=e + 5)
    assert st[3] == 0
    _, st = run_c_call(dm, off, idx, val, ncol=300, row_begin=100, max_rows=1000, max_entries=e - 9)
    assert st[3] == cm.FLAG_MAX_ENTRIES and st[0] + st[1] == e - 9


@pytest.mark.parametrize("index_bits,vt", [(32, "f32"), (64, "f32"), (32, "i64"), (64, "i64"), (32, "i32")])
@pytest.mark.parametrize("ncol", [200, 3000])
def test_types_and_arrays(dm, index_bits, vt, ncol):
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(index_bits + len(vt) + ncol)
    lens = rng.integers(0, 8, size=T // 3)
    off, idx, val = make_csr(rng, lens, ncol + 2, index_bits=index_bits, vt=vt)
    run_c_call(dm, off, idx, val, ncol=ncol, index_bits=index_bits, vt=vt)
    run_c_call(dm, off, idx, val, ncol=ncol, index_bits=index_bits, vt=vt, want_pos=False)
    run_c_call(dm, off, idx, val, ncol=ncol, index_bits=index_bits, vt=vt, want_val=False)
    # no value array: the value output stays unwritten
    got, _ = run_c_call(dm, off, idx, None, ncol=ncol, index_bits=index_bits, vt=vt)
    assert (got["value"] == SENT[_word(vt)]).all()
    run_c_call(dm, off, idx, None, ncol=ncol, index_bits=index_bits, vt=vt, want_val=False, want_pos=False)


def test_capacity(dm):
    rng = np.random.default_rng(10)
    for ncol in (300, 3000):
        off, idx, val = make_csr(rng, rng.integers(0, 8, size=2500), ncol)
        n = len(idx)
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, cap=n - 1)
        assert st == [n, 0, cm.NONE, cm.FLAG_CAPACITY]
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, cap=n // 3)
        assert st == [n, 0, cm.NONE, cm.FLAG_CAPACITY]
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, cap=0)
        assert st == [n, 0, cm.NONE, cm.FLAG_CAPACITY]


def test_flags(dm):
    rng = np.random.default_rng(11)
    for ncol in (300, 3000):
        off, idx, val = make_csr(rng, rng.integers(1, 6, size=400), ncol)
        n = len(idx)
        got, st = run_c_call(dm, off, idx, val, ncol=ncol, error=(123 << 16) | 3)
        assert st == [0, 0, cm.NONE, cm.FLAG_ERROR] and (got["col_offset"][:ncol + 1] == 0).all()
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, counts=(400, n, n - 1))
        assert st == [0, 0, cm.NONE, cm.FLAG_VALUE_COUNT]
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, counts=(400, n, n + 1), error=5)
        assert st == [0, 0, cm.NONE, cm.FLAG_ERROR | cm.FLAG_VALUE_COUNT]
        # offsets past the index capacity: clamped, and the arrays' tail past it never reaches the output
        capi = int(off[250]) - 2
        idx2, val2 = idx.copy(), val.copy()
        idx2[capi:], val2[capi:] = 7, 0xBADBAD
        _, st = run_c_call(dm, off, idx2, val2, ncol=ncol, cap_index=capi)
        assert st[0] == capi and st[3] == cm.FLAG_OFFSET_CAP
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, cap_value=int(off[100]) + 1)
        assert st[0] == int(off[100]) + 1 and st[3] == cm.FLAG_OFFSET_CAP


def test_two_calls_of_different_sizes_through_one_workspace(dm):
    import torch
    T, _ = dm.csc_geometry()
    rng = np.random.default_rng(12)
    big = make_csr(rng, rng.integers(0, 9, size=T), 70000)
    small = make_csr(rng, rng.integers(0, 9, size=200), 300)
    p = dm.CscParams()
    p.index_bits, p.value_type, p.ncol = 32, dm.F32, 70000
    need = dm.lib().dmlc_amd_csc_workspace_bytes(len(big[1]), 70000, ctypes.byref(p))
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda")
    run_c_call(dm, *big, ncol=70000, ws=ws)
    run_c_call(dm, *small, ncol=300, ws=ws)
    run_c_call(dm, *small, ncol=200, ws=ws)
    run_c_call(dm, *big, ncol=70000, ws=ws)
    run_c_call(dm, *big, ncol=256, ws=ws)


# ---------------------------------------------------- after a real parse --
def _parse_cases():
    lib_text = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    csv_text = b"\n".join(b",".join(b"%d" % ((r * 7 + c * 13) % 23 - 11) for c in range(17)) for r in range(200)) + b"\n"
    fm_text = synth.rows(synth.LIBFM, 250, 8, seed=9)[0].tobytes()
    return [("libsvm", lib_text, {}, {}, np.float32),
            ("csv", csv_text, {"label_column": 0, "value_type": "i64"}, {"label_column": 0, "value_kind": po.I64}, np.int64),
            ("libfm", fm_text, {}, {}, np.float32)]


@pytest.fixture(scope="module", params=range(3), ids=["libsvm", "csv-label-i64", "libfm"])
def parsed(request, dm):
    """(parser, device batch, the oracle's CSR), parsed once per format"""
    import torch
    fmt, data, kw, okw, vdt = _parse_cases()[request.param]
    o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt], **okw)
    assert o["status"] == 0
    p = dm.DeviceParser(fmt, flags=dm.FLAG_MAX_INDEX, **kw)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0
    csr = {"offset": np.asarray(o["offset"]).astype(U64), "index": np.asarray(o["index"]).astype(U32),
           "value": np.asarray(o["value"]).astype(vdt), "field": np.asarray(o.get("field", np.zeros(0))).astype(U32),
           "vdt": vdt}
    assert len(csr["index"]) == int(out["counts"][dm.INDEX]) > 0
    return p, out, csr, text, cs


def _model(csr, ncol, offset=None, index=None, value=None):
    offset = csr["offset"] if offset is None else offset
    index = csr["index"] if index is None else index
    value = csr["value"] if value is None else value
    n = len(index)
    vw = U64 if np.dtype(csr["vdt"]).itemsize == 8 else U32
    bufs = {"col_offset": np.zeros(ncol + 1, U64), "row": np.zeros(n, U32), "value": np.zeros(n, vw) if len(value) else None,
            "pos": np.zeros(n, U64)}
    return cm.to_csc(offset, index, value if len(value) else None, bufs,
                     counts=(len(offset) - 1, n, len(value)), ncol=ncol)


def _assert_csc(got, want, wstatus):
    assert [int(x) for x in got["status"]] == wstatus
    kept = wstatus[0]
    assert got["col_offset"].cpu().numpy().view(U64).tobytes() == want["col_offset"].tobytes()
    assert got["row"].cpu().numpy().view(U32).tobytes() == want["row"][:kept].tobytes()
    if want["value"] is None:
        assert got["value"] is None
    else:
        assert cm.bits(got["value"].cpu().numpy()).tobytes() == want["value"][:kept].tobytes()
    if "pos" in got:
        assert got["pos"].cpu().numpy().view(U64).tobytes() == want["pos"][:kept].tobytes()


def test_to_csc_of_a_parse_equals_the_model_over_the_oracle(dm, parsed):
    p, out, csr, _, _ = parsed
    ncol = int(out["max_index"]) + 1
    got = p.to_csc(out, want_pos=True)  # ncol from max_index + 1
    assert got["ncol"] == ncol
    want, wstatus = _model(csr, ncol)
    assert wstatus[1] == 0 and wstatus[0] == len(csr["index"])
    _assert_csc(got, want, wstatus)
    if len(csr["field"]):  # libfm: pos moves the fields
        fields = out["field"][got["pos"]].cpu().numpy().view(U32)
        assert fields.tobytes() == csr["field"][want["pos"].astype(np.int64)].tobytes()
    # fewer columns: the rest is dropped; more columns (several passes): empty columns at the end
    for nc in (max(ncol // 2, 1), ncol + 300):
        want, wstatus = _model(csr, nc)
        _assert_csc(p.to_csc(out, ncol=nc), want, wstatus)


def test_parse_gather_to_csc_on_one_stream_without_a_sync(dm, parsed):
    import torch
    p, out, csr, text, cs = parsed
    rows, nnz = len(csr["offset"]) - 1, len(csr["index"])
    perm = np.random.default_rng(43).permutation(rows)[: rows - 5]
    d_perm = torch.from_numpy(perm).cuda()
    ncol = int(out["max_index"]) + 1
    bound = rows + 50  # upper-bound buffers: every count is read on the device
    ub = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    dst = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    r1 = torch.zeros(16, dtype=torch.int64, device="cuda")
    csc = {"col_offset": torch.full((ncol + 1,), -1, dtype=torch.int64, device="cuda"),
           "row": torch.full((nnz + 50,), -1, dtype=torch.int32, device="cuda"),
           "value": torch.zeros(nnz + 50, dtype=out["value"].dtype, device="cuda"),
           "pos": torch.full((nnz + 50,), -1, dtype=torch.int64, device="cuda")}
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        p.parse_into(text, cs, ub, r1, stream=stream)
        _, r2, gst = p.gather_rows_async(ub, r1, d_perm, dst=dst, stream=stream)
        status = p.to_csc_async(dst, r2, csc, ncol=ncol, stream=stream)
    stream.synchronize()
    # the model over gather_model's output of the oracle's CSR
    vw = U64 if np.dtype(csr["vdt"]).itemsize == 8 else U32
    side = gm.side_from({"offset": csr["offset"], "label": np.zeros(rows, vw), "index": csr["index"],
                         "value": cm.bits(csr["value"]) if len(csr["value"]) else None})
    res = np.zeros(16, dtype=U64)
    res[gm.ROWS] = res[gm.LABEL] = rows
    res[gm.INDEX], res[gm.VALUE] = nnz, len(csr["value"])
    gd = gm.side_from({"offset": np.zeros(len(perm) + 1, U64), "label": np.zeros(len(perm), vw),
                       "index": np.zeros(nnz, U32), "value": np.zeros(nnz, vw)},
                      {gm.ROWS: len(perm), gm.INDEX: nnz, gm.VALUE: nnz})
    g, gres, _ = gm.gather_rows(side, res, perm, gd)
    e = int(gres[gm.INDEX])
    gvalue = g["value"][:e] if len(csr["value"]) else np.zeros(0, vw)
    want, wstatus = _model(csr, ncol, offset=g["offset"][:len(perm) + 1], index=g["index"][:e], value=gvalue)
    assert [int(x) for x in status.cpu().numpy().view(U64)] == wstatus
    kept = wstatus[0]
    assert csc["col_offset"].cpu().numpy().view(U64).tobytes() == want["col_offset"].tobytes()
    assert csc["row"][:kept].cpu().numpy().view(U32).tobytes() == want["row"][:kept].tobytes()
    assert (csc["row"][kept:] == -1).all() and (csc["pos"][kept:] == -1).all()
    if len(csr["value"]):
        assert cm.bits(csc["value"][:kept].cpu().numpy()).tobytes() == want["value"][:kept].tobytes()
    assert csc["pos"][:kept].cpu().numpy().view(U64).tobytes() == want["pos"][:kept].tobytes()


def test_the_csc_scattered_into_a_matrix_is_the_dense_model(dm, parsed):
    """Column c's entries written in order into out[row, c]: the last entry of a cell wins, as in to_dense."""
    p, out, csr, _, _ = parsed
    ncol = int(out["max_index"]) + 1
    rows, nnz = len(csr["offset"]) - 1, len(csr["index"])
    got = p.to_csc(out)
    co = got["col_offset"].cpu().numpy().astype(np.int64)
    row = got["row"].cpu().numpy().astype(np.int64)
    vw = U64 if np.dtype(csr["vdt"]).itemsize == 8 else U32
    fill = 0x7FC01234
    one = {np.dtype(np.float32): 0x3F800000, np.dtype(np.int64): 1}[np.dtype(csr["vdt"])]
    val = cm.bits(got["value"].cpu().numpy()) if got["value"] is not None else np.full(len(row), one, vw)
    mat = np.full((rows, ncol), fill, dtype=vw)
    col = np.repeat(np.arange(ncol), np.diff(co))
    mat[row, col] = val  # (assignment through repeated indices keeps the last)
    buf = np.full(rows * ncol, 0xA5A5A5A5, dtype=vw)
    wdense, _ = dmod.to_dense(csr["offset"], csr["index"], csr["value"], buf, value_dtype=csr["vdt"],
                              counts=(rows, nnz, len(csr["value"])), ncol=ncol, fill_bits=fill)
    assert mat.tobytes() == wdense.tobytes()
