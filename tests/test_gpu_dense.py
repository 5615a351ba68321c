"""GPU tests of dmlc_amd_to_dense: the dense row batch of a parsed CSR, byte for
byte against tests/dense_model.py.

Hand-built CSR tensors go through the C call itself, into a buffer pre-filled
with a sentinel whose every word (padding between ncol and ld, rows past the
window, guard rows) is compared; the edge shapes come from the library's own
tile geometry.  Real parses go through DeviceParser.to_dense / parse_dense
and are compared with the model over the ORACLE's CSR, not the device's."""
import ctypes

import numpy as np
import pytest

import dense_model as dmod
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

SENT32, SENT64 = 0xA5A5A5A5, 0xA5A5A5A5A5A5A5A5
NAN_PAYLOAD = 0x7FC01234
INT64_MIN_BITS = 1 << 63
TYPES = [(ib, vt) for ib in (32, 64) for vt in ("f32", "i32", "i64")]
TYPE_IDS = ["u%d-%s" % t for t in TYPES]
_NP = {"f32": np.float32, "i32": np.int32, "i64": np.int64}


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def _fill_bits(vt):
    return INT64_MIN_BITS if vt == "i64" else NAN_PAYLOAD


def random_csr(rng, rows, ncol, per_row, cmax=None, values=True):
    """rows of 0 .. 2 * per_row random entries (so duplicates and empty rows occur), random value bits"""
    lens = rng.integers(0, 2 * per_row + 1, size=rows) if per_row else np.zeros(rows, np.int64)
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(offset[-1])
    index = rng.integers(0, cmax or ncol, size=nnz, dtype=np.uint64)
    value = rng.integers(0, 1 << 63, size=nnz if values else 0, dtype=np.uint64)
    return offset, index, value


def run_c_call(dm, offset, index, value, *, index_bits, vt, ncol, extra_ld=0, shift=0, row_begin=0, max_rows=None,
               fill_bits=None, counts=None, error=0, cap_rows=None, cap_index=None, guard_rows=2):
    """One dmlc_amd_to_dense over host arrays (index as uint64, value as bit patterns); compares the whole
    output buffer and the status with the model.  Returns the status."""
    import torch
    vdt = _NP[vt]
    word = np.uint64 if vt == "i64" else np.uint32
    idx = index.astype(np.uint32 if index_bits == 32 else np.uint64)
    val = value.astype(word)  # (bit patterns: truncated for the 4-byte types)
    rows = len(offset) - 1
    counts = counts if counts is not None else (rows, len(idx), len(val))
    cap_rows = rows if cap_rows is None else cap_rows
    cap_index = len(idx) if cap_index is None else cap_index
    max_rows = rows if max_rows is None else max_rows
    fill_bits = _fill_bits(vt) if fill_bits is None else fill_bits
    ld = ncol + extra_ld
    buf = np.full(shift + (max_rows + guard_rows) * ld + 4, SENT64 if word is np.uint64 else SENT32, dtype=word)
    dev = torch.device("cuda", 0)
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        {1: np.uint8, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(dev)
    d_off, d_buf = as_t(offset), as_t(buf)
    d_idx = as_t(idx) if len(idx) else torch.zeros(1, dtype=torch.int64, device=dev)
    d_val = as_t(val) if len(val) else torch.zeros(1, dtype=torch.int64, device=dev)
    res = np.zeros(16, dtype=np.uint64)
    res[dm.ROWS], res[dm.INDEX], res[dm.VALUE], res[8] = counts[0], counts[1], counts[2], error
    d_res = as_t(res)
    d_status = torch.full((4,), 0x5555, dtype=torch.int64, device=dev)
    csr = dm.Csr()
    csr.offset, csr.index, csr.value = d_off.data_ptr(), d_idx.data_ptr(), d_val.data_ptr()
    csr.cap[dm.ROWS], csr.cap[dm.INDEX], csr.cap[dm.VALUE] = cap_rows, cap_index, cap_index if len(val) else 0
    p = dm.DenseParams()
    p.index_bits, p.value_type = index_bits, {"f32": dm.F32, "i32": dm.I32, "i64": dm.I64}[vt]
    p.row_begin, p.max_rows, p.ncol, p.ld, p.fill_bits = row_begin, max_rows, ncol, ld, fill_bits
    rc = dm.lib().dmlc_amd_to_dense(ctypes.byref(csr), d_res.data_ptr(), ctypes.byref(p),
                                    d_buf.data_ptr() + shift * buf.dtype.itemsize, d_status.data_ptr(),
                                    torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = d_buf.cpu().numpy().view(word)
    status = [int(x) for x in d_status.cpu().numpy().view(np.uint64)]
    want, wstatus = dmod.to_dense(offset, idx, val.view(vdt), buf, value_dtype=vdt, counts=counts, ncol=ncol,
                                  fill_bits=fill_bits, error=error, cap_rows=cap_rows, cap_index=cap_index,
                                  row_begin=row_begin, max_rows=max_rows, ld=ld, out_shift=shift)
    assert status == wstatus, (status, wstatus)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError("%d words differ, first at %d (row %d col %d): got %#x want %#x"
                             % (len(bad), bad[0], (bad[0] - shift) // ld, (bad[0] - shift) % ld,
                                int(got[bad[0]]), int(want[bad[0]])))
    return status


# ------------------------------------------------------- hand-built CSR --
@pytest.mark.parametrize("index_bits,vt", TYPES, ids=TYPE_IDS)
def test_shapes_strides_and_alignment(dm, index_bits, vt):
    """ncol in {1, 2, 3, 63, 64, 65, C-1, C, C+1, 2C+3} x {0 rows, 1 row, 1 / 2 / 3 row tiles with a partial
    last tile} x {ld == ncol, ld == ncol + 5, out one element into its buffer}."""
    C, R = dm.dense_geometry()
    rng = np.random.default_rng(index_bits * 10 + len(vt))
    for ncol in (1, 2, 3, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3):
        rt = min(R, C // min(ncol, C))  # rows per tile at this width
        for rows in (0, 1, max(rt - 1, 1), rt + 1, 2 * rt + 1):
            per_row = 1 if ncol < 8 else (40 if ncol > 1000 else 6)
            offset, index, value = random_csr(rng, rows, ncol, per_row)
            for extra_ld, shift in ((0, 0), (5, 0), (0, 1)):
                try:
                    st = run_c_call(dm, offset, index, value, index_bits=index_bits, vt=vt, ncol=ncol,
                                    extra_ld=extra_ld, shift=shift)
                except AssertionError as e:
                    raise AssertionError("ncol %d rows %d ld+%d shift %d: %s" % (ncol, rows, extra_ld, shift, e))
                assert st[0] == rows and st[1] == 0 and st[3] == 0


def test_wide_index_is_dropped_not_wrapped(dm):
    rng = np.random.default_rng(5)
    offset, index, value = random_csr(rng, 300, 50, 6)
    index[::7] |= np.uint64(1 << 32)  # low 32 bits < ncol
    for vt in ("f32", "i64"):
        st = run_c_call(dm, offset, index, value, index_bits=64, vt=vt, ncol=50)
        assert st[1] == len(index[::7]) and st[2] == 0


def test_value_and_fill_bits_are_copied_exactly(dm):
    offset = np.array([0, 4, 4, 6], dtype=np.uint64)
    index = np.array([0, 1, 2, 3, 1, 2], dtype=np.uint64)
    f32 = np.array([-0.0, np.nan, np.inf, 1e-45, 0.0, -np.nan], dtype=np.float32).view(np.uint32).astype(np.uint64)
    f32[1] = 0x7FA00001  # a signalling NaN with a payload
    run_c_call(dm, offset, index, f32, index_bits=32, vt="f32", ncol=5, fill_bits=NAN_PAYLOAD)
    run_c_call(dm, offset, index, f32, index_bits=32, vt="f32", ncol=5, fill_bits=0x80000000)  # -0.0
    i64 = np.array([1 << 63, (1 << 63) - 1, 0, (1 << 64) - 1, 5, 1 << 62], dtype=np.uint64)
    run_c_call(dm, offset, index, i64, index_bits=64, vt="i64", ncol=5, fill_bits=INT64_MIN_BITS)
    # the high half of fill_bits is ignored by the 4-byte types
    run_c_call(dm, offset, index, f32, index_bits=32, vt="i32", ncol=5, fill_bits=(0xDEAD << 32) | 0x80000000)


@pytest.mark.parametrize("index_bits,vt", [(32, "f32"), (64, "i64")], ids=["u32-f32", "u64-i64"])
def test_duplicates_last_wins(dm, index_bits, vt):
    """The same cell twice inside one 64-entry stretch, 300 entries apart, and at a 256-entry stride (the same
    thread), in one 700-entry row; then "1 3:1 3:2 3:5"."""
    col = np.arange(700, dtype=np.uint64) % 500
    col[[10, 20, 33]] = 7
    col[[100, 400]] = 450
    col[[5, 261, 517]] = 499
    index = np.concatenate([col, np.array([3, 3, 3], dtype=np.uint64)])
    value = np.concatenate([1000 + np.arange(700, dtype=np.uint64), np.array([1, 2, 5], dtype=np.uint64)])
    offset = np.array([0, 700, 703], dtype=np.uint64)
    for extra_ld in (0, 5):
        run_c_call(dm, offset, index, value, index_bits=index_bits, vt=vt, ncol=500, extra_ld=extra_ld)
    # every entry of a row on one cell: the last of 1000 wins
    offset = np.array([0, 0, 1000, 1000], dtype=np.uint64)
    run_c_call(dm, offset, np.full(1000, 2, dtype=np.uint64), np.arange(1000, dtype=np.uint64) + 1,
               index_bits=index_bits, vt=vt, ncol=3)


def test_row_skew(dm):
    rng = np.random.default_rng(11)
    # one 5000-entry row among 200 empty rows
    lens = np.zeros(201, dtype=np.int64)
    lens[77] = 5000
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    index = rng.integers(0, 300, size=5000, dtype=np.uint64)
    value = rng.integers(0, 1 << 63, size=5000, dtype=np.uint64)
    for extra_ld in (0, 5):
        run_c_call(dm, offset, index, value, index_bits=32, vt="f32", ncol=300, extra_ld=extra_ld)
    # empty first and last rows
    offset, index, value = random_csr(rng, 40, 30, 4)
    offset[1], offset[39] = 0, offset[40]
    run_c_call(dm, offset, index, value, index_bits=32, vt="f32", ncol=30, extra_ld=5)
    run_c_call(dm, offset, index, value, index_bits=64, vt="i64", ncol=30)
    # all rows empty: fill everywhere
    offset, index, value = random_csr(rng, 600, 9, 0)
    st = run_c_call(dm, offset, index, value, index_bits=32, vt="i32", ncol=9)
    assert st[0] == 600


@pytest.mark.parametrize("extra_ld", [0, 5])
def test_row_windows(dm, extra_ld):
    C, R = dm.dense_geometry()
    rng = np.random.default_rng(13)
    ncol = 20
    rt = min(R, C // ncol)
    rows = 3 * rt + 7
    offset, index, value = random_csr(rng, rows, ncol, 5)
    kw = dict(index_bits=32, vt="f32", ncol=ncol, extra_ld=extra_ld)
    # row_begin inside a tile of the whole matrix, to the end
    st = run_c_call(dm, offset, index, value, row_begin=rt // 2 + 1, max_rows=rows - rt // 2 - 1, **kw)
    assert st[0] == rows - rt // 2 - 1
    # max_rows short of the end
    st = run_c_call(dm, offset, index, value, row_begin=7, max_rows=rt + 3, **kw)
    assert st[0] == rt + 3
    # max_rows past the end, in upper-bound buffers: the parsed count ends the window and the tail rows of out
    # keep the sentinel (the model leaves them alone; the comparison covers them)
    big = np.concatenate([offset, np.full(1000, 0xDEAD << 40, dtype=np.uint64)])
    st = run_c_call(dm, big, index, value, row_begin=rows - 50, max_rows=400, counts=(rows, len(index), len(value)),
                    cap_rows=rows + 1000, **kw)
    assert st[0] == 50
    # a window that starts past the parsed rows, and an empty window
    st = run_c_call(dm, big, index, value, row_begin=rows + 10, max_rows=100, counts=(rows, len(index), len(value)),
                    cap_rows=rows + 1000, **kw)
    assert st[0] == 0
    st = run_c_call(dm, offset, index, value, row_begin=3, max_rows=0, **kw)
    assert st == [0, 0, dmod.NONE, 0]


@pytest.mark.parametrize("index_bits,vt", [(32, "f32"), (64, "i32")], ids=["u32-f32", "u64-i32"])
def test_dropped_entries(dm, index_bits, vt):
    C, R = dm.dense_geometry()
    rng = np.random.default_rng(17)
    for ncol, per_row in ((50, 8), (2 * C + 3, 30)):  # (column-tiled: each entry counted once)
        rt = min(R, C // min(ncol, C))
        offset, index, value = random_csr(rng, 2 * rt + 1, ncol, per_row, cmax=ncol + ncol // 4)
        index[:3] = 0  # the first dropped position is not 0
        st = run_c_call(dm, offset, index, value, index_bits=index_bits, vt=vt, ncol=ncol)
        over = np.flatnonzero(index >= ncol)
        assert st[1] == len(over) > 0 and st[2] == over[0] > 0


@pytest.mark.parametrize("index_bits,vt", TYPES, ids=TYPE_IDS)
def test_values_absent_gives_ones(dm, index_bits, vt):
    rng = np.random.default_rng(19)
    offset, index, value = random_csr(rng, 700, 40, 5, values=False)
    for extra_ld in (0, 5):
        run_c_call(dm, offset, index, value, index_bits=index_bits, vt=vt, ncol=40, extra_ld=extra_ld)


def test_error_flags(dm):
    rng = np.random.default_rng(23)
    offset, index, value = random_csr(rng, 400, 20, 5)
    kw = dict(index_bits=32, vt="f32", ncol=20, extra_ld=5)
    # an unequal value count: bit 1, out untouched
    st = run_c_call(dm, offset, index, value, counts=(400, len(index), len(index) - 1), **kw)
    assert st == [0, 0, dmod.NONE, 2]
    # a failed parse: bit 0
    st = run_c_call(dm, offset, index, value, error=(123 << 16) | 3, **kw)
    assert st == [0, 0, dmod.NONE, 1]
    # offsets past cap[INDEX]: bit 2; the arrays' tail past the capacity is a sentinel that must not reach out
    cap = int(offset[250]) - 2
    index2, value2 = index.copy(), value.copy()
    index2[cap:] = 1
    value2[cap:] = 0xBADBADBAD
    st = run_c_call(dm, offset, index2, value2, cap_index=cap, **kw)
    assert st[0] == 400 and st[3] == 4


# ---------------------------------------------------- after a real parse --
def _oracle_dense(o, vdt, ncol, fill_bits, row_begin=0, max_rows=None):
    rows = len(o["offset"]) - 1
    nrow = rows - row_begin if max_rows is None else max_rows
    word = np.uint64 if np.dtype(vdt).itemsize == 8 else np.uint32
    buf = np.full(max(nrow, 0) * ncol, SENT32, dtype=word)
    return dmod.to_dense(o["offset"], o["index"], o["value"].astype(vdt), buf, value_dtype=vdt,
                         counts=(rows, len(o["index"]), len(o["value"])), ncol=ncol, fill_bits=fill_bits,
                         row_begin=row_begin, max_rows=max_rows)


def _parse_cases():
    lib_text = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    csv_text = synth.rows(synth.CSV, 200, 16, seed=9)[0].tobytes()
    fm_text = synth.rows(synth.LIBFM, 100, 8, seed=9)[0].tobytes()
    return [("libsvm", lib_text, {}), ("csv", csv_text, {}),
            ("csv", b"label,f0,f1\n1,2.5,3\n0,,4\n", {"label_column": 0}),
            ("csv", b"1,,3\nnan,2,\n,,\n4,5,6\n-0.0,nan,7\n", {}),
            ("libfm", fm_text, {}),
            ("libsvm", b"1 0 3\n0 2\n1 3 3 1\n", {})]  # no values: ones


@pytest.mark.parametrize("case", range(6), ids=["libsvm", "csv", "csv-label", "csv-empty-nan", "libfm", "novalue"])
def test_after_a_real_parse(dm, case):
    import torch
    fmt, data, kw = _parse_cases()[case]
    o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt], **kw)
    assert o["status"] == 0
    p = dm.DeviceParser(fmt, flags=dm.FLAG_MAX_INDEX, **kw)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0
    nan_bits = dm.fill_bits_of(float("nan"), dm.F32)
    # ncol = max_index + 1 (NumCol): nothing is dropped
    numcol = int(o["index"].max()) + 1
    dense, status = p.to_dense(out)
    want, wstatus = _oracle_dense(o, np.float32, numcol, nan_bits)
    assert tuple(dense.shape) == (len(o["offset"]) - 1, numcol)
    assert [int(x) for x in status] == wstatus and wstatus[1] == 0
    assert dense.cpu().numpy().tobytes() == want.tobytes()
    # a fixed ncol below it: the rest is dropped and counted
    small = max(numcol - 2, 1)
    dense, status = p.to_dense(out, ncol=small, fill=-1.0)
    want, wstatus = _oracle_dense(o, np.float32, small, dm.fill_bits_of(-1.0, dm.F32))
    assert [int(x) for x in status] == wstatus and (wstatus[1] > 0 or small == numcol)
    assert dense.cpu().numpy().tobytes() == want.tobytes()
    # a strided view that starts 3 elements into its buffer
    big = torch.full((len(o["offset"]) - 1, numcol + 5), -7.0, device="cuda")
    status = p.to_dense_async(out, out["result"], big[:, 3:3 + numcol], ncol=numcol, fill_bits=NAN_PAYLOAD)
    torch.cuda.synchronize()
    want, wstatus = _oracle_dense(o, np.float32, numcol, NAN_PAYLOAD)
    got = big.cpu().numpy()
    assert got[:, 3:3 + numcol].tobytes() == want.view(np.float32).reshape(-1, numcol).tobytes()
    assert (got[:, :3] == -7.0).all() and (got[:, 3 + numcol:] == -7.0).all()
    assert [int(x) for x in status.cpu().numpy().view(np.uint64)] == wstatus
    # ncol=None needs FLAG_MAX_INDEX
    with pytest.raises(ValueError):
        dm.DeviceParser(fmt, **kw).to_dense(out)


def test_integer_csv_after_a_real_parse(dm):
    import torch
    data = b"1,-2,3\n,5,\n-9223372036854775808,7,8\n"
    for vt, vdt, kind in (("i32", np.int32, po.I32), ("i64", np.int64, po.I64)):
        o = po.parse_chunks(data, [0, len(data)], fmt=po.CSV, value_kind=kind)
        p = dm.DeviceParser("csv", value_type=vt)
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        out = p.parse(text, torch.tensor([0, len(data)], dtype=torch.int64, device="cuda"))
        fill = -(1 << 63) if vt == "i64" else -(1 << 31)
        dense, status = p.to_dense(out, ncol=3, fill=fill)
        want, wstatus = _oracle_dense(o, vdt, 3, dm.fill_bits_of(fill, p.params.value_type))
        assert dense.cpu().numpy().tobytes() == want.tobytes() and [int(x) for x in status] == wstatus


def test_per_unit_blocks_through_the_chunk_table(dm):
    """Two chunks, nthread=2: each ParseBlock unit's rows are [table[u][ROWS], table[u+1][ROWS]); its dense
    block must be the model on those rows."""
    import torch
    data = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    mid = data.index(b"\n", len(data) // 2) + 1
    offs = [0, mid, len(data)]
    o = po.parse_chunks(data, offs, fmt=po.LIBSVM, nthread=2)
    p = dm.DeviceParser("libsvm", nthread=2, flags=dm.FLAG_MAX_INDEX)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    out = p.parse(text, torch.tensor(offs, dtype=torch.int64, device="cuda"))
    table = out["chunk_table"].cpu().numpy().view(np.uint64).reshape(-1, 8)
    assert table.shape[0] == 4
    bounds = [int(x) for x in table[:, dm.ROWS]] + [int(out["counts"][dm.ROWS])]
    assert bounds[-1] == 300 and bounds == sorted(bounds) and len(set(bounds)) > 2
    ncol = int(o["index"].max()) + 1
    nan_bits = dm.fill_bits_of(float("nan"), dm.F32)
    for u in range(4):
        a, b = bounds[u], bounds[u + 1]
        dense, status = p.to_dense(out, row_begin=a, max_rows=b - a)
        want, wstatus = _oracle_dense(o, np.float32, ncol, nan_bits, row_begin=a, max_rows=b - a)
        assert tuple(dense.shape) == (b - a, ncol) and [int(x) for x in status] == wstatus
        assert dense.cpu().numpy().tobytes() == want.tobytes(), u


def test_parse_dense_equals_the_two_steps(dm):
    import torch
    for fmt, kind, width in (("libsvm", synth.LIBSVM, 20), ("csv", synth.CSV, 16)):
        data = synth.rows(kind, 300, width, seed=4)[0].tobytes()
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
        p = dm.DeviceParser(fmt)
        ncol = 17
        one = p.parse_dense(text, cs, ncol, fill=0.5)
        out = p.parse(text, cs)
        dense, status = p.to_dense(out, ncol=ncol, fill=0.5)
        assert one["error"] == 0 and one["dense"].shape == dense.shape
        assert one["dense"].cpu().numpy().tobytes() == dense.cpu().numpy().tobytes()
        assert list(one["dense_status"]) == list(status) and int(status[0]) == 300
        # the full call into upper-bound outputs with the dense pass queued behind it, no sync in between:
        # the row count is read on the device, rows past it keep what the tensor held
        bound = len(data) // 2 + 2
        ub = p.alloc([bound] * 8)
        res = torch.zeros(16, dtype=torch.int64, device="cuda")
        big = torch.full((bound, ncol), -7.0, device="cuda")
        p.parse_into(text, cs, ub, res)
        st = p.to_dense_async(ub, res, big, ncol=ncol, fill=0.5)
        torch.cuda.synchronize()
        assert int(st[0]) == 300
        assert big[:300].cpu().numpy().tobytes() == dense.cpu().numpy().tobytes()
        assert bool((big[300:] == -7.0).all())
