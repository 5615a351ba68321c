"""CPU-side checks of dmlc_amd_to_dense's C boundary (no GPU needed): every
argument error is returned before any HIP call, the tile geometry is sane and
the parameter block has the header's layout."""
import ctypes

import pytest

ERR_ARG = 32


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    dmlc_amd.lib()
    return dmlc_amd


def _args(dm, **kw):
    csr = dm.Csr()
    # (never dereferenced: every call below must be refused before any device work)
    csr.offset, csr.index, csr.value = 0x1000, 0x2000, 0x3000
    csr.cap[dm.ROWS], csr.cap[dm.INDEX], csr.cap[dm.VALUE] = 10, 100, 100
    p = dm.DenseParams()
    p.index_bits, p.value_type = 32, dm.F32
    p.row_begin, p.max_rows, p.ncol, p.ld, p.fill_bits = 0, 10, 8, 8, 0x7FC00000
    for k, v in kw.items():
        setattr(p, k, v)
    return csr, p


def _call(dm, csr, p, result=0x4000, out=0x5000, status=0x6000):
    return dm.lib().dmlc_amd_to_dense(ctypes.byref(csr) if csr is not None else None, result,
                                      ctypes.byref(p) if p is not None else None, out, status, None)


def test_dense_params_layout(dm):
    assert ctypes.sizeof(dm.DenseParams) == 64
    f = dm.DenseParams
    assert (f.index_bits.offset, f.value_type.offset, f.row_begin.offset, f.max_rows.offset, f.ncol.offset,
            f.ld.offset, f.fill_bits.offset, f.flags.offset, f.reserved.offset) == (0, 4, 8, 16, 24, 32, 40, 48, 52)


def test_geometry_is_sane(dm):
    cells, rows = dm.dense_geometry()
    assert cells >= 1024 and cells & (cells - 1) == 0, cells
    assert 1 <= rows <= cells and rows & (rows - 1) == 0, rows
    # tags (4 bytes a cell) and offsets (8 bytes a row) fit a CU's LDS several times over
    assert cells * 4 + (rows + 1) * 8 <= 64 << 10
    assert dm.lib().dmlc_amd_dense_geometry(None, None) == 0


def test_null_pointers_are_refused(dm):
    csr, p = _args(dm)
    assert _call(dm, None, p) == ERR_ARG
    assert _call(dm, csr, None) == ERR_ARG
    assert _call(dm, csr, p, result=None) == ERR_ARG
    assert _call(dm, csr, p, out=None) == ERR_ARG
    assert _call(dm, csr, p, status=None) == ERR_ARG
    csr.offset = None  # rows to convert but no offsets
    assert _call(dm, csr, p) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(ncol=0, ld=0), dict(ncol=0, ld=8), dict(ncol=8, ld=7), dict(ncol=1 << 40, ld=8),
                                dict(index_bits=16), dict(index_bits=0), dict(value_type=3), dict(value_type=-1)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_bad_shapes_and_types_are_refused(dm, kw):
    csr, p = _args(dm, **kw)
    assert _call(dm, csr, p) == ERR_ARG


def test_unaligned_out_is_refused(dm):
    csr, p = _args(dm)
    assert _call(dm, csr, p, out=0x5002) == ERR_ARG
    csr, p = _args(dm, value_type=dm.I64)
    assert _call(dm, csr, p, out=0x5004) == ERR_ARG


def test_more_tiles_than_a_launch_holds_is_refused_not_truncated(dm):
    cells, rows = dm.dense_geometry()
    limit = (1 << 31) - 1
    # one column: `rows` rows per tile; the capacity allows them all
    csr, p = _args(dm, ncol=1, ld=1, max_rows=(limit + 1) * rows)
    csr.cap[dm.ROWS] = 1 << 62
    assert _call(dm, csr, p) == ERR_ARG
    # column tiles alone
    csr, p = _args(dm, ncol=(limit + 1) * cells, ld=(limit + 1) * cells, max_rows=1)
    assert _call(dm, csr, p) == ERR_ARG
    # rows x column tiles (neither factor too large, and no 64-bit wrap of the product)
    csr, p = _args(dm, ncol=cells << 20, ld=cells << 20, max_rows=1 << 44)
    csr.cap[dm.ROWS] = 1 << 62
    assert _call(dm, csr, p) == ERR_ARG
    csr, p = _args(dm, ncol=cells << 20, ld=cells << 20, max_rows=1 << 12)
    csr.cap[dm.ROWS] = 1 << 62
    assert _call(dm, csr, p) == ERR_ARG


def test_fill_bits_of(dm):
    assert dm.fill_bits_of(float("nan"), dm.F32) & 0x7FC00000 == 0x7FC00000
    assert dm.fill_bits_of(-0.0, dm.F32) == 0x80000000
    assert dm.fill_bits_of(-1, dm.I32) == 0xFFFFFFFF
    assert dm.fill_bits_of(-(1 << 63), dm.I64) == 1 << 63
    with pytest.raises(ValueError):
        dm.fill_bits_of(float("nan"), dm.I64)
