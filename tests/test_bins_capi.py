"""CPU-side checks of dmlc_amd_to_bins's C boundary (no GPU needed): every
argument error is returned before any HIP call, the geometry is sane and the
parameter blocks have the header's layout."""
import ctypes

import pytest

ERR_ARG = 32


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    dmlc_amd.lib()
    return dmlc_amd


def _csr(dm, base=0x100000, cap=100):
    # (never dereferenced: every call below must be refused before any device work)
    c = dm.Csr()
    for i, k in enumerate(("offset", "label", "weight", "qid", "field", "index", "value")):
        setattr(c, k, base + 0x10000 * i)
    for slot in range(7):
        c.cap[slot] = cap
    return c


def _args(dm, **kw):
    p = dm.BinsParams()
    p.index_bits, p.value_type, p.code_bytes, p.missing_code = 32, dm.F32, 1, 255
    p.row_begin, p.max_rows, p.ncol, p.ld, p.flags = 0, 50, 300, 300, 0
    for k, v in kw.items():
        setattr(p, k, v)
    c = dm.Cuts()
    c.cut_ptr, c.cut_value, c.n_cuts = 0x200000, 0x210000, 1000
    return _csr(dm), c, p


def _call(dm, csr, cuts, p, res=0x300000, out=0x400000, status=0x500000):
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return dm.lib().dmlc_amd_to_bins(ref(csr), res, ref(cuts), ref(p), out, status, None)


def test_params_layout(dm):
    f = dm.BinsParams
    assert ctypes.sizeof(f) == 64
    assert (f.index_bits.offset, f.value_type.offset, f.code_bytes.offset, f.missing_code.offset, f.row_begin.offset,
            f.max_rows.offset, f.ncol.offset, f.ld.offset, f.flags.offset, f.reserved.offset) == \
        (0, 4, 8, 12, 16, 24, 32, 40, 48, 52)
    g = dm.Cuts
    assert ctypes.sizeof(g) == 24 and (g.cut_ptr.offset, g.cut_value.offset, g.n_cuts.offset) == (0, 8, 16)


def test_geometry_is_sane(dm):
    C, R = dm.bins_geometry()
    assert C >= 256 and C % 256 == 0 and 1 <= R <= C, (C, R)
    assert dm.lib().dmlc_amd_bins_geometry(None, None) == 0
    assert "dmlc_amd_to_bins" in dm.EXPORTED_SYMBOLS and "dmlc_amd_bins_geometry" in dm.EXPORTED_SYMBOLS


def test_null_pointers_are_refused(dm):
    csr, cuts, p = _args(dm)
    assert _call(dm, None, cuts, p) == ERR_ARG
    assert _call(dm, csr, None, p) == ERR_ARG
    assert _call(dm, csr, cuts, None) == ERR_ARG
    assert _call(dm, csr, cuts, p, res=None) == ERR_ARG
    assert _call(dm, csr, cuts, p, out=None) == ERR_ARG
    assert _call(dm, csr, cuts, p, status=None) == ERR_ARG
    csr, cuts, p = _args(dm)
    cuts.cut_ptr = None
    assert _call(dm, csr, cuts, p) == ERR_ARG
    csr, cuts, p = _args(dm)
    cuts.cut_value = None  # (null only with n_cuts == 0)
    assert _call(dm, csr, cuts, p) == ERR_ARG
    # a window with rows needs the offsets, and the indices when there can be any
    for name in ("offset", "index"):
        csr, cuts, p = _args(dm)
        setattr(csr, name, None)
        assert _call(dm, csr, cuts, p) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(ncol=0), dict(ncol=1 << 32, ld=1 << 32), dict(ncol=(1 << 64) - 1, ld=(1 << 64) - 1),
                                dict(ld=299), dict(ld=0), dict(index_bits=16), dict(index_bits=0),
                                dict(value_type=1), dict(value_type=2), dict(value_type=3), dict(value_type=-1),
                                dict(code_bytes=0), dict(code_bytes=3), dict(code_bytes=8), dict(code_bytes=-1),
                                dict(code_bytes=1, missing_code=256), dict(code_bytes=1, missing_code=0xFFFFFFFF),
                                dict(code_bytes=2, missing_code=65536), dict(flags=2), dict(flags=3),
                                dict(flags=1 << 31)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_bad_shapes_types_codes_and_flags_are_refused(dm, kw):
    csr, cuts, p = _args(dm, **kw)
    assert _call(dm, csr, cuts, p) == ERR_ARG


@pytest.mark.parametrize("word", [0, 1, 2])
def test_a_nonzero_reserved_word_is_refused(dm, word):
    csr, cuts, p = _args(dm)
    p.reserved[word] = 1
    assert _call(dm, csr, cuts, p) == ERR_ARG


@pytest.mark.parametrize("code_bytes,shift", [(2, 1), (4, 1), (4, 2), (4, 3)])
def test_an_output_not_aligned_to_its_element_is_refused(dm, code_bytes, shift):
    csr, cuts, p = _args(dm, code_bytes=code_bytes, missing_code=0)
    assert _call(dm, csr, cuts, p, out=0x400000 + shift) == ERR_ARG


@pytest.mark.parametrize("which", ["out", "status"])
@pytest.mark.parametrize("src", ["offset", "label", "weight", "qid", "field", "index", "value", "result", "cut_ptr",
                                 "cut_value"])
def test_an_output_that_is_a_source_array_is_refused(dm, which, src):
    csr, cuts, p = _args(dm)
    ptr = 0x300000 if src == "result" else getattr(cuts, src) if src.startswith("cut_") else getattr(csr, src)
    assert _call(dm, csr, cuts, p, **{which: ptr}) == ERR_ARG


def test_a_window_of_more_tiles_than_one_launch_is_refused(dm):
    C, R = dm.bins_geometry()
    # ncol = C: one row per tile, so 2^31 rows are 2^31 tiles
    csr, cuts, p = _args(dm, ncol=C, ld=C, max_rows=1 << 31)
    csr.cap[dm.ROWS] = 1 << 31
    assert _call(dm, csr, cuts, p) == ERR_ARG
    # column tiles times row tiles
    csr, cuts, p = _args(dm, ncol=C * 4096, ld=C * 4096, max_rows=1 << 20)
    csr.cap[dm.ROWS] = 1 << 20
    assert _call(dm, csr, cuts, p) == ERR_ARG
