"""GPU tests of dmlc_amd_to_bins: the quantised dense row batch of a parsed CSR,
byte for byte against tests/bins_model.py.

Hand-built CSR tensors go through the C call itself, into a buffer pre-filled
with a sentinel whose every element (padding between ncol and ld, rows past
the window, guard rows, the bytes before a shifted out) is compared; the edge
shapes come from the library's own tile geometry.  Real parses go through
DeviceParser.to_bins / parse_bins and are compared with the model over the
ORACLE's CSR, not the device's."""
import ctypes

import numpy as np
import pytest

import bins_model as bmod
import gather_model as gm
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

SENT = {1: 0xA5, 2: 0xA5A5, 4: 0xA5A5A5A5}
WORD = {1: np.uint8, 2: np.uint16, 4: np.uint32}
NAN_PAYLOAD = 0x7FC01234
CUT_COUNTS = (0, 1, 2, 3, 255, 256, 257)
WIDTHS = [(ib, cb) for ib in (32, 64) for cb in (1, 2, 4)]
WIDTH_IDS = ["u%d-c%d" % w for w in WIDTHS]
SPECIALS = np.array([0x00000000, 0x80000000, 0x7F800000, 0xFF800000, 0x00000001, NAN_PAYLOAD],
                    dtype=np.uint32)  # +0, -0, +inf, -inf, the smallest denormal, NaN with a payload


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def make_cuts(rng, ncol, menu=CUT_COUNTS):
    """cut_ptr (uint32[ncol + 1]) and ascending float32 cuts per column (equal neighbours occur), counts from menu"""
    m = rng.choice(np.asarray(menu), size=ncol)
    cut_ptr = np.concatenate([[0], np.cumsum(m)]).astype(np.uint32)
    steps = rng.integers(0, 4, size=int(cut_ptr[-1])).astype(np.float32) * np.float32(0.25)
    start = rng.integers(-100, 100, size=ncol).astype(np.float32)
    cuts = np.cumsum(steps, dtype=np.float64)
    base = np.repeat(cuts[np.minimum(cut_ptr[:-1], max(len(cuts) - 1, 0))] if len(cuts) else np.zeros(ncol), m)
    cut_value = (cuts - base + np.repeat(start, m)).astype(np.float32)
    return cut_ptr, cut_value


def menu_for(ncol):
    # (every count at small widths; wide matrices mostly few cuts, so the table stays small)
    return CUT_COUNTS if ncol <= 65 else (0, 1, 2, 3) * 12 + (255, 256, 257)


def draw_values(rng, index, ncol, cut_ptr, cut_value):
    """value bits per entry: one of the column's cuts, nextafter of one in either direction, a special, or a value
    below the first / above the last cut"""
    n = len(index)
    col = np.minimum(index, ncol - 1).astype(np.int64)
    b, e = cut_ptr[col].astype(np.int64), cut_ptr[col + 1].astype(np.int64)
    m = np.maximum(e - b, 1)
    q = cut_value[np.minimum(b + rng.integers(0, 1 << 30, size=n) % m, max(len(cut_value) - 1, 0))] \
        if len(cut_value) else np.zeros(n, np.float32)
    kind = rng.integers(0, 6, size=n)
    v = np.where(kind == 1, np.nextafter(q, np.float32(np.inf)), q)
    v = np.where(kind == 2, np.nextafter(q, np.float32(-np.inf)), v).astype(np.float32)
    v = np.where(kind == 3, np.float32(-1e30), v)
    v = np.where(kind == 4, np.float32(1e30), v).astype(np.float32)
    bits = v.view(np.uint32).copy()
    sp = kind == 5
    bits[sp] = SPECIALS[rng.integers(0, len(SPECIALS), size=int(sp.sum()))]
    return bits


def random_csr(rng, rows, ncol, per_row, cut_ptr, cut_value, cmax=None, values=True):
    """rows of 0 .. 2 * per_row random entries (so duplicates and empty rows occur)"""
    lens = rng.integers(0, 2 * per_row + 1, size=rows) if per_row else np.zeros(rows, np.int64)
    offset = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
    nnz = int(offset[-1])
    index = rng.integers(0, cmax or ncol, size=nnz, dtype=np.uint64)
    value = draw_values(rng, index, ncol, cut_ptr, cut_value) if values else np.zeros(0, np.uint32)
    return offset, index, value


def run_c_call(dm, offset, index, value, cut_ptr, cut_value, *, index_bits, code_bytes, ncol, extra_ld=0, shift=0,
               row_begin=0, max_rows=None, missing=None, global_ids=False, counts=None, error=0, cap_rows=None,
               cap_index=None, n_cuts=None, guard_rows=2):
    """One dmlc_amd_to_bins over host arrays (index as uint64, value as float bit patterns); compares the whole
    output buffer and the status with the model.  Returns (status, codes of the window as rows x ncol)."""
    import torch
    word = WORD[code_bytes]
    idx = index.astype(np.uint32 if index_bits == 32 else np.uint64)
    val = value.astype(np.uint32)
    rows = len(offset) - 1
    counts = counts if counts is not None else (rows, len(idx), len(val))
    cap_rows = rows if cap_rows is None else cap_rows
    cap_index = len(idx) if cap_index is None else cap_index
    max_rows = rows if max_rows is None else max_rows
    missing = (1 << (8 * code_bytes)) - 1 if missing is None else missing
    n_cuts = len(cut_value) if n_cuts is None else n_cuts
    ld = ncol + extra_ld
    buf = np.full(shift + (max_rows + guard_rows) * ld + 4, SENT[code_bytes], dtype=word)
    dev = torch.device("cuda", 0)
    as_t = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(  # noqa: E731
        {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}[a.dtype.itemsize])).to(dev)
    d_off, d_buf = as_t(offset), as_t(buf)
    d_idx = as_t(idx) if len(idx) else torch.zeros(1, dtype=torch.int64, device=dev)
    d_val = as_t(val) if len(val) else torch.zeros(1, dtype=torch.int64, device=dev)
    d_ptr = as_t(np.asarray(cut_ptr, dtype=np.uint32))
    d_cut = as_t(np.asarray(cut_value, dtype=np.float32)) if len(cut_value) else \
        torch.zeros(1, dtype=torch.int32, device=dev)
    res = np.zeros(16, dtype=np.uint64)
    res[dm.ROWS], res[dm.INDEX], res[dm.VALUE], res[8] = counts[0], counts[1], counts[2], error
    d_res = as_t(res)
    d_status = torch.full((8,), 0x5555, dtype=torch.int64, device=dev)
    csr = dm.Csr()
    csr.offset, csr.index, csr.value = d_off.data_ptr(), d_idx.data_ptr(), d_val.data_ptr()
    csr.cap[dm.ROWS], csr.cap[dm.INDEX], csr.cap[dm.VALUE] = cap_rows, cap_index, cap_index if len(val) else 0
    c = dm.Cuts()
    c.cut_ptr, c.cut_value, c.n_cuts = d_ptr.data_ptr(), d_cut.data_ptr(), n_cuts
    p = dm.BinsParams()
    p.index_bits, p.value_type, p.code_bytes, p.missing_code = index_bits, dm.F32, code_bytes, missing
    p.row_begin, p.max_rows, p.ncol, p.ld = row_begin, max_rows, ncol, ld
    p.flags = dm.BINS_GLOBAL if global_ids else 0
    rc = dm.lib().dmlc_amd_to_bins(ctypes.byref(csr), d_res.data_ptr(), ctypes.byref(c), ctypes.byref(p),
                                   d_buf.data_ptr() + shift * code_bytes, d_status.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream)
    assert rc == 0, rc
    torch.cuda.synchronize()
    got = d_buf.cpu().numpy().view(word)
    status = [int(x) for x in d_status.cpu().numpy().view(np.uint64)]
    want, wstatus = bmod.to_bins(offset, idx, val.view(np.float32), buf, cut_ptr, cut_value, counts=counts, ncol=ncol,
                                 n_cuts=n_cuts, missing=missing, global_ids=global_ids, error=error,
                                 cap_rows=cap_rows, cap_index=cap_index, row_begin=row_begin, max_rows=max_rows,
                                 ld=ld, out_shift=shift)
    assert status == wstatus, (status, wstatus)
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got != want)
        raise AssertionError("%d elements differ, first at %d (row %d col %d): got %#x want %#x"
                             % (len(bad), bad[0], (bad[0] - shift) // ld, (bad[0] - shift) % ld,
                                int(got[bad[0]]), int(want[bad[0]])))
    nrow = status[0]
    codes = np.lib.stride_tricks.as_strided(got[shift:], shape=(nrow, ncol),
                                            strides=(ld * code_bytes, code_bytes)).copy() if nrow else None
    return status, codes


# ------------------------------------------------------- hand-built CSR --
@pytest.mark.parametrize("index_bits,code_bytes", WIDTHS, ids=WIDTH_IDS)
def test_shapes_strides_and_alignment(dm, index_bits, code_bytes):
    """ncol in {1, 2, 3, 15, 16, 17, 63, 64, 65, C-1, C, C+1, 2C+3} x {0 rows, 1 row, 1 / 2 / 3 row tiles with a
    partial last tile} x {ld == ncol, ld == ncol + 5, out shifted by 1, 3 and 15 elements}, cut counts mixed from
    {0, 1, 2, 3, 255, 256, 257}, values on and around the cuts."""
    C, R = dm.bins_geometry()
    rng = np.random.default_rng(index_bits * 10 + code_bytes)
    seen = set()
    for ncol in (1, 2, 3, 15, 16, 17, 63, 64, 65, C - 1, C, C + 1, 2 * C + 3):
        rt = min(R, C // min(ncol, C))  # rows per tile at this width
        cut_ptr, cut_value = make_cuts(rng, ncol, menu_for(ncol))
        for rows in (0, 1, max(rt - 1, 1), rt + 1, 2 * rt + 1):
            per_row = 1 if ncol < 8 else (40 if ncol > 1000 else 6)
            offset, index, value = random_csr(rng, rows, ncol, per_row, cut_ptr, cut_value)
            for extra_ld, shift in ((0, 0), (5, 0), (0, 1), (0, 3), (0, 15)):
                try:
                    st, _ = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=index_bits,
                                       code_bytes=code_bytes, ncol=ncol, extra_ld=extra_ld, shift=shift)
                except AssertionError as e:
                    raise AssertionError("ncol %d rows %d ld+%d shift %d: %s" % (ncol, rows, extra_ld, shift, e))
                assert st[0] == rows and st[1] == 0 and st[3] & 15 == 0
                seen.add((st[4] > 0, st[5] > 0))
    assert (True, True) in seen  # NaN cells and unbinned cells occurred


def test_each_special_value_against_each_cut_count(dm):
    """+-0, +-inf, the smallest denormal, a NaN with a payload, every cut itself and its two neighbours, in columns
    of 1, 2, 3, 255, 256, 257 cuts that contain 0.0 -- one row per value, every column the same value."""
    cols = []
    for m in (1, 2, 3, 255, 256, 257):
        q = (np.arange(m, dtype=np.float32) - np.float32(m // 2)) * np.float32(0.5)  # ascending, holds 0.0
        cols.append(q)
    cut_ptr = np.concatenate([[0], np.cumsum([len(q) for q in cols])]).astype(np.uint32)
    cut_value = np.concatenate(cols)
    probe = np.unique(np.concatenate([cut_value, np.nextafter(cut_value, np.float32(np.inf)),
                                      np.nextafter(cut_value, np.float32(-np.inf))]))
    bits = np.concatenate([SPECIALS, probe.view(np.uint32)])
    ncol = len(cols)
    offset = (np.arange(len(bits) + 1) * ncol).astype(np.uint64)
    index = np.tile(np.arange(ncol, dtype=np.uint64), len(bits))
    value = np.repeat(bits, ncol)
    st, codes = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=32, code_bytes=2, ncol=ncol)
    assert st[4] == ncol and st[5] == 0 and st[3] == 0
    # spelled out for the specials: -0.0 == 0.0 sits on the cut 0.0 at position m // 2 -> code min(m // 2 + 1, m - 1)
    for c, m in enumerate((1, 2, 3, 255, 256, 257)):
        zero = min(m // 2 + 1, m - 1)
        assert [int(x) for x in codes[:6, c]] == [zero, zero, m - 1, 0, zero, 0xFFFF], (m, codes[:6, c])


def test_code_range(dm):
    rng = np.random.default_rng(3)
    for m, missing, flagged in ((257, 255, True), (256, 255, True), (255, 255, False), (256, 0, True)):
        ncol = 6
        cut_ptr, cut_value = make_cuts(rng, ncol, (m,))
        offset, index, value = random_csr(rng, 40, ncol, 4, cut_ptr, cut_value)
        value[::3] = np.float32(1e30).view(np.uint32)  # the top code m - 1
        value[1::3] = np.float32(-1e30).view(np.uint32)  # code 0
        st, codes = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=32, code_bytes=1, ncol=ncol,
                               missing=missing)
        assert bool(st[3] & bmod.FLAG_CODE_RANGE) == flagged, (m, missing, st)
        if m == 257:  # no byte holds 256: those cells read missing_code
            assert int(codes.max()) == 255
        # the same cuts in two bytes: nothing to flag
        st, codes = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=32, code_bytes=2, ncol=ncol)
        assert st[3] == 0 and int(np.where(codes == 0xFFFF, 0, codes).max()) == m - 1


def test_cut_ptr_flag_and_the_capacity_of_the_cuts(dm):
    rng = np.random.default_rng(4)
    C, _ = dm.bins_geometry()
    for ncol in (12, C + 9):
        cut_ptr, _ = make_cuts(rng, ncol, (1, 2, 3))
        # one ascending table, so that whatever range a column owns is ascending
        cut_value = (np.arange(int(cut_ptr[-1]) + 4, dtype=np.float32) * np.float32(0.25) - np.float32(20))
        offset, index, value = random_csr(rng, 30, ncol, 60 if ncol > 1000 else 8, cut_ptr, cut_value)
        index[:3] = (5, ncol - 1, ncol - 2)  # the columns below hold entries
        # descending at column 5 (column 6 then starts inside column 4's cuts)
        desc = cut_ptr.copy()
        desc[6] = desc[5] - 1
        st, _ = run_c_call(dm, offset, index, value, desc, cut_value, index_bits=32, code_bytes=1, ncol=ncol)
        assert st[3] == bmod.FLAG_CUT_PTR and st[5] > 0
        # cut_ptr[c + 1] > n_cuts for the last two columns; the floats past n_cuts are NaN and must not matter
        n_cuts = int(cut_ptr[ncol - 2])
        guarded = cut_value.copy()
        guarded[n_cuts:] = np.array([NAN_PAYLOAD], dtype=np.uint32).view(np.float32)[0]
        st, codes = run_c_call(dm, offset, index, value, cut_ptr, guarded, index_bits=64, code_bytes=2, ncol=ncol,
                               n_cuts=n_cuts, extra_ld=5)
        assert st[3] == bmod.FLAG_CUT_PTR and st[5] > 0
        # the usable columns' codes are those of the unguarded table
        st2, codes2 = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=64, code_bytes=2,
                                 ncol=ncol, extra_ld=5)
        assert st2[3] == 0 and (codes[:, :ncol - 2] == codes2[:, :ncol - 2]).all()


def test_error_flags_write_nothing(dm):
    rng = np.random.default_rng(23)
    cut_ptr, cut_value = make_cuts(rng, 20)
    offset, index, value = random_csr(rng, 400, 20, 5, cut_ptr, cut_value)
    kw = dict(index_bits=32, code_bytes=1, ncol=20, extra_ld=5)
    # an unequal value count: bit 1, out untouched (the whole buffer is compared with the model's untouched one)
    st, _ = run_c_call(dm, offset, index, value, cut_ptr, cut_value, counts=(400, len(index), len(index) - 1), **kw)
    assert st == [0, 0, bmod.NONE, 2, 0, 0, 0, 0]
    # a failed parse: bit 0
    st, _ = run_c_call(dm, offset, index, value, cut_ptr, cut_value, error=(123 << 16) | 3, **kw)
    assert st == [0, 0, bmod.NONE, 1, 0, 0, 0, 0]
    # offsets past cap[INDEX]: bit 2; the arrays' tail past the capacity is a sentinel that must not reach out
    cap = int(offset[250]) - 2
    index2, value2 = index.copy(), value.copy()
    index2[cap:] = 1
    value2[cap:] = np.float32(1e30).view(np.uint32)
    st, _ = run_c_call(dm, offset, index2, value2, cut_ptr, cut_value, cap_index=cap, **kw)
    assert st[0] == 400 and st[3] & 15 == 4


@pytest.mark.parametrize("extra_ld", [0, 5])
def test_row_windows(dm, extra_ld):
    C, R = dm.bins_geometry()
    rng = np.random.default_rng(13)
    ncol = 20
    rt = min(R, C // ncol)
    rows = 3 * rt + 7
    cut_ptr, cut_value = make_cuts(rng, ncol, (0, 1, 2, 3, 16))
    offset, index, value = random_csr(rng, rows, ncol, 5, cut_ptr, cut_value)
    kw = dict(index_bits=32, code_bytes=1, ncol=ncol, extra_ld=extra_ld)
    call = lambda off, **k: run_c_call(dm, off, index, value, cut_ptr, cut_value, **k, **kw)[0]  # noqa: E731
    # row_begin inside a tile of the whole matrix, to the end
    assert call(offset, row_begin=rt // 2 + 1, max_rows=rows - rt // 2 - 1)[0] == rows - rt // 2 - 1
    # max_rows short of the end
    assert call(offset, row_begin=7, max_rows=rt + 3)[0] == rt + 3
    # max_rows past the parsed rows, in upper-bound buffers: the parsed count ends the window and the tail rows
    # of out keep the sentinel (the model leaves them alone; the comparison covers them)
    big = np.concatenate([offset, np.full(1000, 0xDEAD << 40, dtype=np.uint64)])
    n = (rows, len(index), len(value))
    assert call(big, row_begin=rows - 50, max_rows=400, counts=n, cap_rows=rows + 1000)[0] == 50
    # a window that starts past the parsed rows, and an empty window
    assert call(big, row_begin=rows + 10, max_rows=100, counts=n, cap_rows=rows + 1000)[0] == 0
    assert call(offset, row_begin=3, max_rows=0) == [0, 0, bmod.NONE, 0, 0, 0, 0, 0]


@pytest.mark.parametrize("index_bits,code_bytes", WIDTHS, ids=WIDTH_IDS)
def test_values_absent_gives_the_code_of_one(dm, index_bits, code_bytes):
    rng = np.random.default_rng(19)
    ncol = 40
    cut_ptr, cut_value = make_cuts(rng, ncol, (1, 2, 3, 16))
    offset, index, value = random_csr(rng, 700, ncol, 5, cut_ptr, cut_value, values=False)
    one = [int(bmod.search_bin(cut_value[cut_ptr[c]:cut_ptr[c + 1]], np.float32(1.0))) for c in range(ncol)]
    for extra_ld in (0, 5):
        st, codes = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=index_bits,
                               code_bytes=code_bytes, ncol=ncol, extra_ld=extra_ld)
        top = (1 << (8 * code_bytes)) - 1
        assert ((codes == top) | (codes == np.asarray(one)[None, :])).all() and (codes != top).any()


def test_dropped_entries_and_wide_indices(dm):
    C, R = dm.bins_geometry()
    rng = np.random.default_rng(17)
    for ncol, per_row in ((50, 8), (2 * C + 3, 30)):  # (column-tiled: each entry counted once)
        rt = min(R, C // min(ncol, C))
        cut_ptr, cut_value = make_cuts(rng, ncol, menu_for(ncol))
        offset, index, value = random_csr(rng, 2 * rt + 1, ncol, per_row, cut_ptr, cut_value, cmax=ncol + ncol // 4)
        index[:3] = 0  # the first dropped position is not 0
        st, _ = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=32, code_bytes=1, ncol=ncol)
        over = np.flatnonzero(index >= ncol)
        assert st[1] == len(over) > 0 and st[2] == over[0] > 0
    index[::7] |= np.uint64(1 << 32)  # low 32 bits < ncol: dropped, not wrapped
    st, _ = run_c_call(dm, offset, index, value, cut_ptr, cut_value, index_bits=64, code_bytes=2, ncol=ncol)
    assert st[1] >= len(index[::7])


def test_global_ids_are_local_codes_plus_cut_ptr(dm):
    rng = np.random.default_rng(29)
    C, _ = dm.bins_geometry()
    for ncol, rows in ((65, 300), (C + 9, 5)):
        cut_ptr, cut_value = make_cuts(rng, ncol, menu_for(ncol))
        offset, index, value = random_csr(rng, rows, ncol, 6 if ncol < 100 else 200, cut_ptr, cut_value)
        kw = dict(index_bits=32, code_bytes=4, ncol=ncol)
        st, local = run_c_call(dm, offset, index, value, cut_ptr, cut_value, **kw)
        stg, glob = run_c_call(dm, offset, index, value, cut_ptr, cut_value, global_ids=True, **kw)
        assert st == stg and st[3] == 0
        miss = 0xFFFFFFFF
        want = np.where(local == miss, miss, local.astype(np.int64) + cut_ptr[:-1].astype(np.int64)[None, :])
        assert (glob == want).all() and (local != miss).any()


# ---------------------------------------------------- after a real parse --
def quantile_cuts(o, ncol, nbins=16):
    """per-column quantiles of the oracle's CSR values (NaNs aside), as ascending unique float32 cuts"""
    idx, val = np.asarray(o["index"]).astype(np.int64), np.asarray(o["value"]).astype(np.float32)
    cols = []
    for c in range(ncol):
        v = val[idx == c] if len(val) else np.ones(int((idx == c).sum()), np.float32)
        v = v[~np.isnan(v)]
        cols.append(np.unique(np.quantile(v, np.linspace(0, 1, nbins + 1)[:-1]).astype(np.float32))
                    if len(v) else np.zeros(0, np.float32))
    cut_ptr = np.concatenate([[0], np.cumsum([len(q) for q in cols])]).astype(np.uint32)
    return cut_ptr, np.concatenate(cols).astype(np.float32) if cols else np.zeros(0, np.float32)


def _oracle_bins(o, ncol, cut_ptr, cut_value, word=np.uint8, row_begin=0, max_rows=None, **kw):
    rows = len(o["offset"]) - 1
    nrow = rows - row_begin if max_rows is None else max_rows
    buf = np.full(max(nrow, 0) * ncol, 0xA5, dtype=word)
    return bmod.to_bins(o["offset"], o["index"], np.asarray(o["value"]).astype(np.float32), buf, cut_ptr, cut_value,
                        counts=(rows, len(o["index"]), len(o["value"])), ncol=ncol, row_begin=row_begin,
                        max_rows=max_rows, **kw)


def _parse_cases():
    lib_text = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    lib_dup = lib_text + b"1 0:7 3:1 3:2 3:-5\n0 3:9 3:0.5 19:1e30 19:-1e30\n"  # duplicate cells
    csv_text = synth.rows(synth.CSV, 200, 16, seed=9)[0].tobytes()
    fm_text = synth.rows(synth.LIBFM, 100, 8, seed=9)[0].tobytes()
    return [("libsvm", lib_dup, {}), ("csv", csv_text, {}),
            ("csv", b"label,f0,f1\n1,2.5,3\n0,,4\n", {"label_column": 0}),
            ("csv", b"1,,3\nnan,2,\n,,\n4,5,6\n-0.0,nan,7\n", {}),  # NaN cells
            ("libfm", fm_text, {}),
            ("libsvm", b"1 0 3\n0 2\n1 3 3 1\n", {})]  # no values: ones


def _to_dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int32)).cuda()


@pytest.mark.parametrize("case", range(6), ids=["libsvm-dup", "csv", "csv-label", "csv-empty-nan", "libfm", "novalue"])
def test_after_a_real_parse(dm, case):
    import torch
    fmt, data, kw = _parse_cases()[case]
    o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt], **kw)
    assert o["status"] == 0
    p = dm.DeviceParser(fmt, **kw)
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    out = p.parse(text, cs)
    assert out["error"] == 0
    ncol = int(np.asarray(o["index"]).max()) + 1
    rows = len(o["offset"]) - 1
    cut_ptr, cut_value = quantile_cuts(o, ncol)
    d_ptr, d_cut = _to_dev(cut_ptr), _to_dev(cut_value).view(torch.float32)
    bins, status = p.to_bins(out, d_ptr, d_cut)
    want, wstatus = _oracle_bins(o, ncol, cut_ptr, cut_value)
    assert tuple(bins.shape) == (rows, ncol) and bins.dtype == torch.uint8
    assert [int(x) for x in status] == wstatus and wstatus[1] == 0 and wstatus[3] == 0
    assert bins.cpu().numpy().tobytes() == want.tobytes()
    # two-byte codes with global ids, fewer columns (the rest is dropped and counted), a row window
    small = max(ncol - 2, 1)
    bins, status = p.to_bins(out, d_ptr, d_cut, ncol=small, dtype=torch.int16, global_ids=True, row_begin=1,
                             max_rows=rows - 1, missing=0x7FFF)
    want, wstatus = _oracle_bins(o, small, cut_ptr, cut_value, word=np.uint16, global_ids=True, row_begin=1,
                                 max_rows=rows - 1, missing=0x7FFF)
    assert [int(x) for x in status] == wstatus and (wstatus[1] > 0 or small == ncol)
    assert bins.cpu().numpy().tobytes() == want.tobytes()
    # a strided view that starts 3 elements into its buffer
    big = torch.full((rows, ncol + 5), 77, dtype=torch.uint8, device="cuda")
    status = p.to_bins_async(out, out["result"], big[:, 3:3 + ncol], d_ptr, d_cut, ncol=ncol)
    torch.cuda.synchronize()
    want, wstatus = _oracle_bins(o, ncol, cut_ptr, cut_value)
    got = big.cpu().numpy()
    assert got[:, 3:3 + ncol].tobytes() == want.tobytes()
    assert (got[:, :3] == 77).all() and (got[:, 3 + ncol:] == 77).all()
    assert [int(x) for x in status.cpu().numpy().view(np.uint64)] == wstatus
    # parse_bins: count, then write pass and bins pass on one stream
    one = p.parse_bins(text, cs, d_ptr, d_cut, ncol)
    assert one["error"] == 0 and [int(x) for x in one["bins_status"]] == wstatus
    assert one["bins"].cpu().numpy().tobytes() == want.tobytes()


def test_to_bins_equals_the_search_over_to_dense(dm):
    import torch
    for fmt, kind, width in (("libsvm", synth.LIBSVM, 20), ("csv", synth.CSV, 16)):
        data = synth.rows(kind, 300, width, seed=4)[0].tobytes()
        o = po.parse_chunks(data, [0, len(data)], fmt=dm._FMT[fmt])
        p = dm.DeviceParser(fmt)
        text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
        out = p.parse(text, torch.tensor([0, len(data)], dtype=torch.int64, device="cuda"))
        ncol = int(np.asarray(o["index"]).max()) + 1
        cut_ptr, cut_value = quantile_cuts(o, ncol, nbins=32)
        bins, status = p.to_bins(out, _to_dev(cut_ptr), _to_dev(cut_value).view(torch.float32))
        dense, dstatus = p.to_dense(out, ncol=ncol, fill_bits=NAN_PAYLOAD)
        d = dense.cpu().numpy()
        present = d.view(np.uint32) != NAN_PAYLOAD  # (the texts hold no NaN)
        codes, n_nan, n_unb, flags = bmod.codes_of(d, present, cut_ptr, cut_value)
        assert bins.cpu().numpy().tobytes() == codes.astype(np.uint8).tobytes()
        assert [int(x) for x in status[:4]] == [int(x) for x in dstatus] and int(status[3]) == flags == 0
        assert (int(status[4]), int(status[5])) == (n_nan, n_unb)


def test_parse_gather_to_bins_on_one_stream_without_a_sync(dm):
    """parse -> gather_rows_async(perm) -> to_bins_async queued back to back; the codes must be the bins model
    over the model's gathered CSR of the oracle's parse."""
    import torch
    data = synth.rows(synth.LIBSVM, 300, 20, seed=9)[0].tobytes()
    o = po.parse_chunks(data, [0, len(data)], fmt=po.LIBSVM)
    p = dm.DeviceParser("libsvm")
    text = torch.frombuffer(bytearray(data), dtype=torch.uint8).cuda()
    cs = torch.tensor([0, len(data)], dtype=torch.int64, device="cuda")
    typed = {"offset": np.asarray(o["offset"]).astype(np.uint64), "label": np.asarray(o["label"]).astype(np.float32),
             "weight": np.asarray(o["weight"]).astype(np.float32), "qid": np.asarray(o["qid"]).astype(np.uint64),
             "field": np.zeros(0, np.uint32), "index": np.asarray(o["index"]).astype(np.uint32),
             "value": np.asarray(o["value"]).astype(np.float32)}
    side = gm.side_from({k: gm.bits(v) if len(v) else None for k, v in typed.items()})
    rows, nnz = len(typed["offset"]) - 1, len(typed["index"])
    res = np.zeros(16, dtype=np.uint64)
    res[gm.ROWS] = rows
    for k, slot in (("label", gm.LABEL), ("weight", gm.WEIGHT), ("qid", gm.QID), ("index", gm.INDEX),
                    ("value", gm.VALUE)):
        res[slot] = len(typed[k])
    ncol = int(typed["index"].max()) + 1
    cut_ptr, cut_value = quantile_cuts(o, ncol)
    perm = np.random.default_rng(43).permutation(rows)[: rows - 5]
    bound = rows + 50  # upper-bound buffers: every count is read on the device
    sizes = [bound, nnz + 50, nnz + 50, bound, bound, bound, nnz + 50, 0]
    ub, dst = p.alloc(sizes), p.alloc(sizes)
    r1 = torch.zeros(16, dtype=torch.int64, device="cuda")
    bins = torch.full((bound, ncol), 77, dtype=torch.uint8, device="cuda")
    d_perm, d_ptr, d_cut = torch.from_numpy(perm).cuda(), _to_dev(cut_ptr), _to_dev(cut_value).view(torch.float32)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        p.parse_into(text, cs, ub, r1, stream=stream)
        _, r2, gst = p.gather_rows_async(ub, r1, d_perm, dst=dst, stream=stream)
        bst = p.to_bins_async(dst, r2, bins, d_ptr, d_cut, ncol=ncol, stream=stream)
    stream.synchronize()
    n = len(perm)
    word = {"offset": np.uint64, "label": np.uint32, "weight": np.uint32, "qid": np.uint64, "field": np.uint32,
            "index": np.uint32, "value": np.uint32}
    gdst = gm.side_from({k: np.zeros(n + 1 if k == "offset" else (n if k in ("label", "weight", "qid") else nnz),
                                     dtype=word[k]) for k in gm.ARRAYS})
    want, wres, wstatus = gm.gather_rows(side, res, perm, gdst)
    assert [int(x) for x in gst.cpu().numpy().view(np.uint64)] == wstatus
    e = wres[gm.INDEX]
    buf = np.full(n * ncol, 0xA5, dtype=np.uint8)
    wbins, wbstatus = bmod.to_bins(want["offset"][:n + 1], want["index"][:e], want["value"][:e].view(np.float32), buf,
                                   cut_ptr, cut_value, counts=(n, e, wres[gm.VALUE]), ncol=ncol)
    assert [int(x) for x in bst.cpu().numpy().view(np.uint64)] == wbstatus
    got = bins.cpu().numpy()
    assert got[:n].tobytes() == wbins.tobytes()
    assert (got[n:] == 77).all()
