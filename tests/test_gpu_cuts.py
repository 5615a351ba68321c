"""GPU tests of dmlc_amd_make_cuts: per-column quantile cut points of a CSR's
row window, word for word against tests/cuts_model.py.

Hand-built CSR goes through the C call itself.  cut_ptr and cut_value are
pre-filled with 0xA5.. and the workspace with 0xCD; every output word is
compared with the model, guard words past ncol + 1 and past the capacity
included, and all eight status words.  The edge shapes come from the library's
own geometry (T entries per tile); nothing is larger than 257T + 3 entries.
Real parses go through DeviceParser.make_cuts / make_cuts_async and are
compared with the model over the ORACLE's CSR.  Nothing has a tolerance: every
comparison is of bit patterns."""
import ctypes

import numpy as np
import pytest

import bins_model as bm
import cuts_model as qm
import gather_model as gm
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

U32, U64 = np.uint32, np.uint64
GUARD = 3
SENT = 0xA5A5A5A5


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def values(rng, n, distinct=False):
    """float bits: finite, mostly from a pool of 40 values (ties) unless distinct"""
    b = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(U32)
    b[(b & U32(0x7F800000)) == U32(0x7F800000)] &= U32(0xBFFFFFFF)
    if not distinct:
        pool = ((rng.integers(0, 40, size=n) - 20) * 0.25).astype(np.float32).view(U32)
        b = np.where(rng.integers(0, 3, size=n) > 0, pool, b)
    return b


def make_csr(rng, lens, ncol_max, *, index_bits=32, value=True, distinct=False):
    lens = np.asarray(lens, dtype=np.int64)
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(U64)
    nnz = int(offset[-1])
    index = rng.integers(0, ncol_max, size=nnz, dtype=np.uint64).astype(U32 if index_bits == 32 else U64)
    return offset, index, values(rng, nnz, distinct) if value else None


def lens_for(rng, n, hi=9):
    """row lengths of 0 .. hi summing to exactly n"""
    lens = []
    left = n
    while left > 0:
        m = min(int(rng.integers(0, hi + 1)), left)
        lens.append(m)
        left -= m
    return lens + [0, 0]


def run_c_call(dm, offset, index, value, *, ncol, max_bin=256, index_bits=32, counts=None, row_begin=0, max_rows=None,
               cap=None, cap_rows=None, cap_index=None, cap_value=None, error=0, max_entries=0, ws=None, runs=1):
    """One dmlc_amd_make_cuts over host arrays; compares every output word and the status with the model.
    cap=None is exactly N_CUTS, a negative cap is that many short of it.  Returns (outputs, status)."""
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
    kw = dict(counts=counts, ncol=ncol, max_bin=max_bin, error=error, cap_rows=cap_rows, cap_index=cap_index,
              cap_value=cap_value, row_begin=row_begin, max_rows=max_rows, max_entries=max_entries)
    if cap is None or cap < 0:  # relative to what the walk emits
        big = {"cut_ptr": np.zeros(ncol + 1, U32), "cut_value": np.zeros(nnz + 1, U32)}
        n_cuts = qm.make_cuts(offset, index, value, big, **kw)[1][qm.N_CUTS]
        cap = max(n_cuts + (cap or 0), 0)
    bufs = {"cut_ptr": np.full(ncol + 1 + GUARD, SENT, U32), "cut_value": np.full(cap + GUARD, SENT, U32), "cap": cap}
    want, wstatus = qm.make_cuts(offset, index, value, bufs, **kw)
    d_off = as_t(offset)
    d_idx = as_t(index if nnz else np.zeros(1, it))
    d_val = as_t(value if value is not None and nnz else np.zeros(1, U32))
    res = np.zeros(16, dtype=U64)
    res[dm.ROWS], res[dm.INDEX], res[dm.VALUE], res[8] = counts[0], counts[1], counts[2], error
    d_res = as_t(res)
    csr = dm.Csr()
    csr.offset, csr.index = d_off.data_ptr(), d_idx.data_ptr()
    csr.value = d_val.data_ptr() if value is not None else None
    csr.cap[dm.ROWS], csr.cap[dm.INDEX], csr.cap[dm.VALUE] = cap_rows, cap_index, cap_value
    p = dm.MakeCutsParams()
    p.index_bits, p.value_type = index_bits, dm.F32
    p.row_begin, p.max_rows = row_begin, (1 << 64) - 1 if max_rows is None else max_rows
    p.ncol, p.max_entries, p.max_bin = ncol, max_entries, max_bin
    need = dm.lib().dmlc_amd_make_cuts_workspace_bytes(min(max_entries, cap_index) if max_entries else cap_index, ncol,
                                                       ctypes.byref(p))
    assert need > 0
    if ws is None:
        ws = torch.full((need,), 0xCD, dtype=torch.uint8, device=dev)
    assert ws.numel() >= need
    first = None
    for _ in range(runs):
        d_out = {k: as_t(bufs[k]) for k in ("cut_ptr", "cut_value")}
        d_status = torch.full((8,), 0x5555, dtype=torch.int64, device=dev)
        c = dm.CutsOut()
        c.cut_ptr, c.cut_value, c.cap = d_out["cut_ptr"].data_ptr(), d_out["cut_value"].data_ptr(), cap
        rc = dm.lib().dmlc_amd_make_cuts(ctypes.byref(csr), d_res.data_ptr(), ctypes.byref(p), ctypes.byref(c),
                                         d_status.data_ptr(), ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
        torch.cuda.synchronize()
        status = [int(x) for x in d_status.cpu().numpy().view(U64)]
        got = {k: t.cpu().numpy().view(U32) for k, t in d_out.items()}
        if first is None:
            first = (got, status)
        else:  # the same bytes on every run
            assert status == first[1] and all(got[k].tobytes() == first[0][k].tobytes() for k in got)
    got, status = first
    print("ncol %d max_bin %d entries %d cap %d status %s" % (ncol, max_bin, nnz, cap, status))
    assert status == wstatus, (status, wstatus)
    for k in got:
        if got[k].tobytes() != want[k].tobytes():
            bad = np.flatnonzero(got[k] != want[k])
            raise AssertionError("%s: %d words differ, first at %d of %d (capacity %d): got %#x want %#x"
                                 % (k, len(bad), bad[0], len(got[k]), cap, int(got[k][bad[0]]), int(want[k][bad[0]])))
    return got, status


# ------------------------------------------------------- hand-built CSR --
def test_entry_counts_around_the_tile_size(dm):
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(1)
    for n in (0, 1, T - 1, T, T + 1, 2 * T + 1):
        off, idx, val = make_csr(rng, lens_for(rng, n), 210)
        _, st = run_c_call(dm, off, idx, val, ncol=200)
        assert st[0] + st[1] == n and st[3] == 0, n


def test_scan_run_longer_than_one_tile_and_the_same_bytes_twice(dm):
    """257 T + 3 entries: each thread of the scan walks two tiles."""
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(2)
    n = 257 * T + 3
    lens = np.full(n // 37 + 1, 37)
    lens[-1] = n - 37 * (n // 37)
    off, idx, val = make_csr(rng, lens, 256, distinct=True)
    _, st = run_c_call(dm, off, idx, val, ncol=256, runs=2)
    assert st[:4] == [n, 0, qm.NONE, 0] and st[qm.N_CUTS] == 256 * 256


@pytest.mark.parametrize("ncol,npass", [(1, 5), (2, 5), (255, 5), (256, 5), (257, 6), (65536, 6), (65537, 7)])
def test_ncol_and_the_pass_count(dm, ncol, npass):
    T, _ = dm.make_cuts_geometry()
    assert qm.passes(ncol) == npass
    rng = np.random.default_rng(ncol)
    off, idx, val = make_csr(rng, rng.integers(0, 9, size=T // 4 + 100), ncol + (3 if ncol > 2 else 1))
    if ncol > 200:  # the top columns are there, and entries just past them
        idx[:3] = [ncol - 1, ncol - 2, 0]
        idx[10:13] = [ncol, ncol + 1, ncol + 2]
    got, st = run_c_call(dm, off, idx, val, ncol=ncol, runs=2)
    assert st[0] + st[1] == len(idx) > T and st[0] > 0 and st[1] > 0  # (more than one tile)
    if ncol > 200:
        assert got["cut_ptr"][ncol] - got["cut_ptr"][ncol - 1] >= 1
        # empty columns first, last and in the middle
        idx[(idx == 0) | (idx == ncol - 1) | (idx == ncol // 2)] = 1
        got, st = run_c_call(dm, off, idx, val, ncol=ncol)
        p = got["cut_ptr"].astype(np.int64)
        assert p[1] == 0 and p[ncol] == p[ncol - 1] and p[ncol // 2 + 1] == p[ncol // 2] and st[qm.EMPTY_COLS] >= 3


@pytest.mark.parametrize("max_bin", [1, 2, 3, 255, 256, 257, 4096])
def test_max_bin_below_at_and_above_a_workgroup(dm, max_bin):
    rng = np.random.default_rng(max_bin)
    off, idx, val = make_csr(rng, rng.integers(0, 9, size=2500), 5)
    val[idx == 3] = values(rng, int((idx == 3).sum()), distinct=True)
    got, st = run_c_call(dm, off, idx, val, ncol=5, max_bin=max_bin)
    p = got["cut_ptr"].astype(np.int64)
    assert 1 <= p[4] - p[3] <= max_bin and p[4] - p[3] >= min(max_bin, 250)  # the distinct column fills its bins


@pytest.mark.parametrize("B", [16, 256])
def test_columns_of_few_samples_and_an_all_equal_column(dm, B):
    rng = np.random.default_rng(B)
    ns = [1, 2, B - 1, B, B + 1, 0, 3 * B + 7]
    idx = np.repeat(np.arange(7), ns).astype(U32)
    val = values(rng, len(idx), distinct=True)
    val[idx == 6] = np.float32(2.5).view(U32)
    perm = rng.permutation(len(idx))
    idx, val = idx[perm], val[perm]
    off = np.concatenate([[0], np.cumsum(lens_for(rng, len(idx)))]).astype(U64)
    got, st = run_c_call(dm, off, idx, val, ncol=8, max_bin=B)
    p = got["cut_ptr"].astype(np.int64)
    assert np.diff(p[:9]).tolist()[5:] == [0, 1, 0] and st[qm.EMPTY_COLS] == 2


def test_one_column_of_3T_plus_5_among_columns_of_one(dm):
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(5)
    n = 3 * T + 5
    idx = np.full(n + 299, 77, U32)
    idx[rng.choice(n + 299, 299, replace=False)] = np.delete(np.arange(300), 77).astype(U32)
    val = values(rng, len(idx))
    off = np.concatenate([[0], np.cumsum(lens_for(rng, len(idx), 30))]).astype(U64)
    _, st = run_c_call(dm, off, idx, val, ncol=300)
    assert st[0] == n + 299 and st[qm.EMPTY_COLS] == 0


@pytest.mark.parametrize("byte", [0, 1, 2, 3])
def test_keys_that_differ_in_one_byte_only(dm, byte):
    rng = np.random.default_rng(byte)
    n = 900
    val = (U32(0x40000000) ^ (rng.integers(0, 0x3F if byte == 3 else 0x100, size=n).astype(U32) << U32(8 * byte)))
    idx = rng.integers(0, 3, size=n).astype(U32)
    off = np.concatenate([[0], np.cumsum(lens_for(rng, n))]).astype(U64)
    _, st = run_c_call(dm, off, idx, val, ncol=3)
    assert st[qm.N_CUTS] > 60  # the byte's values tell the samples apart


@pytest.mark.parametrize("ncol", [300, 70000])
def test_keys_that_tie_across_columns(dm, ncol):
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(ncol)
    n = 2 * T + 1
    pool = np.array([-3, -0.5, 0, 1, 7], np.float32).view(U32)
    val = pool[rng.integers(0, 5, size=n)]
    idx = (rng.integers(0, 40, size=n) * (ncol // 40) + rng.integers(0, 2, size=n) * 3).astype(U32)
    off = np.concatenate([[0], np.cumsum(lens_for(rng, n))]).astype(U64)
    _, st = run_c_call(dm, off, idx, val, ncol=ncol, max_bin=16)
    assert st[0] == n and st[qm.N_CUTS] == 80 * 5


@pytest.mark.parametrize("B", [4, 256])
def test_float_edges(dm, B):
    pz, nz, pinf, ninf, fmax = 0, 0x80000000, 0x7F800000, 0xFF800000, 0x7F7FFFFF
    nan1, nan2, nan3, nan4 = 0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF
    one, two = 0x3F800000, 0x40000000
    cols = [[nz, pz], [fmax], [ninf], [pinf], [ninf, pinf, one, one | nz],
            [1, 2, 0x80000001, 0x80000002, 0x007FFFFF, 0x807FFFFF], [0x80000001, one | nz, two | nz],
            [nan1, nan2, nan3, nan4], [nan1, pinf, two, nan2], [nz, nz, nz], [], [pz, one, two, pz, one, two, two],
            [fmax, 0xFF7FFFFF, pinf, ninf, nan4], [0x00800000, 0x80800000, pz]]
    idx = np.concatenate([np.full(len(c), i) for i, c in enumerate(cols)] * 3).astype(U32)
    val = np.concatenate([np.array(c, U32) for c in cols] * 3)
    rng = np.random.default_rng(B)
    off = np.concatenate([[0], np.cumsum(lens_for(rng, len(idx)))]).astype(U64)
    got, st = run_c_call(dm, off, idx, val, ncol=len(cols), max_bin=B)
    p, v = got["cut_ptr"].astype(np.int64), got["cut_value"]
    assert st[qm.NAN] == 3 * 7 and st[qm.EMPTY_COLS] == 2
    assert v[p[0]:p[1]].tolist() == [1] and v[p[1]:p[2]].tolist() == [pinf] and v[p[2]:p[3]].tolist() == [0xFF7FFFFF]
    assert v[p[3]:p[4]].tolist() == [pinf] and v[p[7] - 1] == 0 and v[p[10] - 1] == 1


def test_dropped_entries_and_64_bit_indices(dm):
    rng = np.random.default_rng(6)
    off, idx, val = make_csr(rng, rng.integers(1, 7, size=2000), 100)
    idx[7], idx[3], idx[500] = 100, 101, 0xFFFFFFFF
    _, st = run_c_call(dm, off, idx, val, ncol=100)
    assert st[1] == 3 and st[2] == 3
    # 64-bit indices: 2^32 + c must not become a sample of column c
    off, idx, val = make_csr(rng, rng.integers(1, 7, size=2000), 100, index_bits=64)
    idx[2], idx[600], idx[9] = (1 << 32) + 5, (1 << 32) + 99, (1 << 63) + 1
    _, st = run_c_call(dm, off, idx, val, ncol=100, index_bits=64)
    assert st[1] == 3 and st[2] == 2
    # every entry dropped
    idx[:] = idx + np.uint64(100)
    _, st = run_c_call(dm, off, idx, val, ncol=100, index_bits=64)
    assert st[0] == 0 and st[1] == len(idx) and st[2] == 0 and st[qm.N_CUTS] == 0 and st[qm.EMPTY_COLS] == 100


def test_absent_values_and_row_windows(dm):
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(9)
    off, idx, _ = make_csr(rng, rng.integers(0, 8, size=500), 303, value=False)
    got, st = run_c_call(dm, off, idx, None, ncol=300)
    n = st[qm.N_CUTS]
    assert n == 300 - st[qm.EMPTY_COLS] and (got["cut_value"][:n] == 0x3F800001).all()  # one cut a column, just above 1
    lens = rng.integers(0, 8, size=T)
    off, idx, val = make_csr(rng, lens, 303)
    rows = len(lens)
    for ncol in (300, 70000):
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, row_begin=rows // 3 + 1)  # begins inside a tile
        assert 0 < st[0] < len(idx)
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, row_begin=17, max_rows=rows // 2)  # max_rows cuts a tile
        assert 0 < st[0] < len(idx)
        for kw in (dict(max_rows=0), dict(row_begin=rows), dict(row_begin=rows + 5, max_rows=3)):
            assert run_c_call(dm, off, idx, val, ncol=ncol, **kw)[1] == [0, 0, qm.NONE, 0, 0, 0, ncol, 0]
    run_c_call(dm, off, idx, val, ncol=300, cap_rows=rows - 500)
    e = int(off[1100] - off[100])
    _, st = run_c_call(dm, off, idx, val, ncol=300, row_begin=100, max_rows=1000, max_entries=e)
    assert st[3] == 0
    _, st = run_c_call(dm, off, idx, val, ncol=300, row_begin=100, max_rows=1000, max_entries=e - 1)
    assert st[3] == qm.FLAG_MAX_ENTRIES and st[0] + st[1] == e - 1


def test_capacity(dm):
    rng = np.random.default_rng(10)
    for ncol, B in ((300, 256), (3000, 4096)):
        off, idx, val = make_csr(rng, rng.integers(0, 8, size=2500), ncol)
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, max_bin=B)  # exactly N_CUTS
        n = st[qm.N_CUTS]
        assert st[3] == 0 and n > ncol // 2
        for cap in (-1, -(2 * n // 3)):
            _, st = run_c_call(dm, off, idx, val, ncol=ncol, max_bin=B, cap=cap)
            assert st[3] == qm.FLAG_CAPACITY and st[qm.N_CUTS] == n
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, max_bin=B, cap=0)
        assert st[3] == qm.FLAG_CAPACITY and st[qm.N_CUTS] == n
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, max_bin=B, cap=n + 2)
        assert st[3] == 0


def test_flags(dm):
    rng = np.random.default_rng(11)
    for ncol in (300, 3000):
        off, idx, val = make_csr(rng, rng.integers(1, 6, size=400), ncol)
        n = len(idx)
        none = [0, 0, qm.NONE, 0, 0, 0, ncol, 0]
        got, st = run_c_call(dm, off, idx, val, ncol=ncol, error=(123 << 16) | 3, cap=50)
        assert st == none[:3] + [qm.FLAG_ERROR] + none[4:] and (got["cut_ptr"][:ncol + 1] == 0).all()
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, counts=(400, n, n - 1), cap=50)
        assert st[3] == qm.FLAG_VALUE_COUNT
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, counts=(400, n, n + 1), error=5, cap=50)
        assert st[3] == qm.FLAG_ERROR | qm.FLAG_VALUE_COUNT
        # offsets past the index capacity: clamped, and the arrays' tail past it never becomes a sample
        capi = int(off[250]) - 2
        idx2, val2 = idx.copy(), val.copy()
        idx2[capi:], val2[capi:] = 7, np.float32(1e30).view(U32)
        _, st = run_c_call(dm, off, idx2, val2, ncol=ncol, cap_index=capi)
        assert st[0] == capi and st[3] == qm.FLAG_OFFSET_CAP
        _, st = run_c_call(dm, off, idx, val, ncol=ncol, cap_value=int(off[100]) + 1)
        assert st[0] == int(off[100]) + 1 and st[3] == qm.FLAG_OFFSET_CAP


def test_two_calls_of_different_sizes_through_one_workspace(dm):
    import torch
    T, _ = dm.make_cuts_geometry()
    rng = np.random.default_rng(12)
    big = make_csr(rng, rng.integers(0, 9, size=T), 70000)
    small = make_csr(rng, rng.integers(0, 9, size=200), 300)
    p = dm.MakeCutsParams()
    p.index_bits, p.value_type, p.ncol, p.max_bin = 32, dm.F32, 70000, 256
    need = dm.lib().dmlc_amd_make_cuts_workspace_bytes(len(big[1]), 70000, ctypes.byref(p))
    ws = torch.full((need,), 0xCD, dtype=torch.uint8, device="cuda")
    run_c_call(dm, *big, ncol=70000, ws=ws)
    run_c_call(dm, *small, ncol=300, ws=ws)
    run_c_call(dm, *small, ncol=200, max_bin=7, ws=ws)
    run_c_call(dm, *big, ncol=70000, ws=ws)
    run_c_call(dm, *big, ncol=256, ws=ws)


# ---------------------------------------------------- after a real parse --
def _parse_cases():
    lib_text = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    csv_text = b"\n".join(b",".join(b"%d.%d" % ((r * 7 + c * 13) % 23 - 11, (r * c) % 4) for c in range(17))
                          for r in range(200)) + b"\n"
    fm_text = synth.rows(synth.LIBFM, 250, 8, seed=9)[0].tobytes()
    return [("libsvm", lib_text, {}, {}), ("csv", csv_text, {"label_column": 0}, {"label_column": 0}), ("libfm", fm_text, {}, {})]


@pytest.fixture(scope="module", params=range(3), ids=["libsvm", "csv-label", "libfm"])
def parsed(request, dm):
    """(parser, device batch, the oracle's CSR), parsed once per format"""
    import torch
    fmt, data, kw, okw = _parse_cases()[request.param]
    o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt], **okw)
    assert o["status"] == 0
    p = dm.DeviceParser(fmt, flags=dm.FLAG_MAX_INDEX, **kw)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0
    csr = {"offset": np.asarray(o["offset"]).astype(U64), "index": np.asarray(o["index"]).astype(U32),
           "value": np.asarray(o["value"]).astype(np.float32)}
    assert len(csr["index"]) == int(out["counts"][dm.INDEX]) > 0
    return p, out, csr, text, cs


def _model(offset, index, value, ncol, max_bin, cap=None, **kw):
    n = len(index)
    cap = n if cap is None else cap
    bufs = {"cut_ptr": np.zeros(ncol + 1, U32), "cut_value": np.zeros(cap, U32), "cap": cap}
    return qm.make_cuts(offset, index, value if len(value) else None, bufs, counts=(len(offset) - 1, n, len(value)),
                        ncol=ncol, max_bin=max_bin, **kw)


def test_make_cuts_of_a_parse_equals_the_model_over_the_oracle(dm, parsed):
    p, out, csr, _, _ = parsed
    ncol = int(out["max_index"]) + 1
    for kw in (dict(), dict(max_bin=16), dict(max_bin=3, row_begin=50, max_rows=120), dict(ncol=max(ncol // 2, 1)),
               dict(ncol=ncol + 300, max_bin=2)):
        cut_ptr, cut_value, status = p.make_cuts(out, **kw)  # ncol from max_index + 1
        mkw = dict(kw)
        want, wstatus = _model(csr["offset"], csr["index"], csr["value"], mkw.pop("ncol", ncol), mkw.pop("max_bin", 256),
                               **mkw)
        assert [int(x) for x in status] == wstatus, kw
        assert cut_ptr.cpu().numpy().view(U32).tobytes() == want["cut_ptr"].tobytes(), kw
        n = wstatus[qm.N_CUTS]
        assert cut_value.numel() == n and cut_value.cpu().numpy().view(U32).tobytes() == want["cut_value"][:n].tobytes(), kw


def test_parse_gather_make_cuts_to_bins_on_one_stream_without_a_sync(dm, parsed):
    import torch
    p, out, csr, text, cs = parsed
    rows, nnz = len(csr["offset"]) - 1, len(csr["index"])
    perm = np.random.default_rng(43).permutation(rows)[: rows - 5]
    d_perm = torch.from_numpy(perm).cuda()
    ncol = int(out["max_index"]) + 1 + 2  # (two columns without a sample)
    B = 16
    bound = rows + 50  # upper-bound buffers: every count is read on the device
    ub = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    dst = p.alloc([bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0])
    r1 = torch.zeros(16, dtype=torch.int64, device="cuda")
    cap = ncol * B
    cut_ptr = torch.full((ncol + 1,), -1, dtype=torch.int32, device="cuda")
    cut_value = torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda")
    bins = torch.full((len(perm) + 3, ncol), 77, dtype=torch.uint8, device="cuda")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        p.parse_into(text, cs, ub, r1, stream=stream)
        _, r2, gst = p.gather_rows_async(ub, r1, d_perm, dst=dst, stream=stream)
        cst = p.make_cuts_async(dst, r2, cut_ptr, cut_value, ncol=ncol, max_bin=B, max_rows=40, stream=stream)  # a sample
        bst = p.to_bins_async(dst, r2, bins, cut_ptr, cut_value, ncol=ncol, stream=stream)  # n_cuts = cap
    stream.synchronize()
    # the models over gather_model's output of the oracle's CSR
    side = gm.side_from({"offset": csr["offset"], "label": np.zeros(rows, U32), "index": csr["index"],
                         "value": csr["value"].view(U32) if len(csr["value"]) else None})
    res = np.zeros(16, dtype=U64)
    res[gm.ROWS] = res[gm.LABEL] = rows
    res[gm.INDEX], res[gm.VALUE] = nnz, len(csr["value"])
    gd = gm.side_from({"offset": np.zeros(len(perm) + 1, U64), "label": np.zeros(len(perm), U32),
                       "index": np.zeros(nnz, U32), "value": np.zeros(nnz, U32)},
                      {gm.ROWS: len(perm), gm.INDEX: nnz, gm.VALUE: nnz})
    g, gres, _ = gm.gather_rows(side, res, perm, gd)
    e = int(gres[gm.INDEX])
    goff, gidx = g["offset"][:len(perm) + 1], g["index"][:e]
    gval = g["value"][:e].view(np.float32) if len(csr["value"]) else np.zeros(0, np.float32)
    want, wstatus = _model(goff, gidx, gval, ncol, B, cap=cap, max_rows=40)
    assert [int(x) for x in cst.cpu().numpy().view(U64)] == wstatus
    n = wstatus[qm.N_CUTS]
    assert wstatus[qm.EMPTY_COLS] >= 2 and 0 < n <= cap
    assert cut_ptr.cpu().numpy().view(U32).tobytes() == want["cut_ptr"].tobytes()
    got_v = cut_value.cpu().numpy().view(U32)
    assert got_v[:n].tobytes() == want["cut_value"][:n].tobytes() and (got_v[n:] == 0x7FC00000).all()
    buf = np.full(bins.numel(), 77, np.uint8)
    wbins, wbst = bm.to_bins(goff, gidx, gval if len(gval) else None, buf, want["cut_ptr"], want["cut_value"].view(np.float32),
                             counts=(len(perm), e, len(gval)), ncol=ncol, n_cuts=cap)
    assert [int(x) for x in bst.cpu().numpy().view(U64)] == wbst
    assert bins.cpu().numpy().tobytes() == wbins.tobytes()
    # UNBINNED: exactly the cells of the columns without cuts
    p64 = want["cut_ptr"].astype(np.int64)
    empty = np.flatnonzero(np.diff(p64) == 0)
    grow = np.repeat(np.arange(len(perm)), np.diff(goff.astype(np.int64)))
    cells = np.unique(np.stack([grow, gidx.astype(np.int64)]), axis=1)
    assert wbst[bm.UNBINNED] == int(np.isin(cells[1], empty).sum()) and wbst[bm.NAN] == 0


def test_occupancy_end_to_end(dm):
    """1024 rows whose column values are permutations of 1024 distinct numbers, max_bin = 16: every code 0 .. 15
    appears exactly 64 times in every column."""
    import torch
    rng = np.random.default_rng(7)
    ncol = 9
    cols = [rng.permutation(1024) * (c + 1) - 300 * c for c in range(ncol)]
    data = b"\n".join(b",".join(b"%d.5" % cols[c][r] for c in range(ncol)) for r in range(1024)) + b"\n"
    p = dm.DeviceParser("csv")
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0 and int(out["counts"][dm.ROWS]) == 1024
    cut_ptr, cut_value, status = p.make_cuts(out, ncol=ncol, max_bin=16)
    assert [int(x) for x in status] == [1024 * ncol, 0, qm.NONE, 0, 0, 16 * ncol, 0, 0]
    assert cut_ptr.cpu().numpy().tolist() == [16 * c for c in range(ncol + 1)]
    bins, bst = p.to_bins(out, cut_ptr, cut_value, ncol=ncol, dtype=torch.uint8)
    assert int(bst[bm.UNBINNED]) == 0 and int(bst[bm.NAN]) == 0
    codes = bins.cpu().numpy()
    for c in range(ncol):
        assert np.bincount(codes[:, c], minlength=16).tolist() == [64] * 16, c
