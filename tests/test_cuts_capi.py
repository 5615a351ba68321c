"""CPU-side checks of dmlc_amd_make_cuts's C boundary (no GPU needed): every
argument error is returned before any HIP call, the geometry and the workspace
size are sane and the parameter blocks have the header's layout."""
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
    p = dm.MakeCutsParams()
    p.index_bits, p.value_type, p.row_begin, p.max_rows, p.ncol, p.max_entries = 32, dm.F32, 0, 50, 300, 0
    p.max_bin, p.flags = 256, 0
    for k, v in kw.items():
        setattr(p, k, v)
    c = dm.CutsOut()
    c.cut_ptr, c.cut_value, c.cap = 0x200000, 0x210000, 100
    return _csr(dm), p, c


def _ws(dm, p, m=100):
    q = dm.MakeCutsParams.from_buffer_copy(p)
    q.ncol = min(max(int(q.ncol), 1), 1 << 20)
    q.max_bin = min(max(int(q.max_bin), 1), 4096)
    q.index_bits, q.value_type, q.flags = 32, dm.F32, 0
    for i in range(2):
        q.reserved[i] = 0
    return dm.lib().dmlc_amd_make_cuts_workspace_bytes(m, q.ncol, ctypes.byref(q))


def _call(dm, csr, p, c, res=0x300000, status=0x400000, ws=0x500000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = max(_ws(dm, p), 1) if p is not None else 1 << 20
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return dm.lib().dmlc_amd_make_cuts(ref(csr), res, ref(p), ref(c), status, ws, ws_bytes, None)


def test_params_layout_and_exports(dm):
    f = dm.MakeCutsParams
    assert ctypes.sizeof(f) == 56
    assert (f.index_bits.offset, f.value_type.offset, f.row_begin.offset, f.max_rows.offset, f.ncol.offset,
            f.max_entries.offset, f.max_bin.offset, f.flags.offset, f.reserved.offset) == (0, 4, 8, 16, 24, 32, 40, 44, 48)
    g = dm.CutsOut
    assert ctypes.sizeof(g) == 24 and (g.cut_ptr.offset, g.cut_value.offset, g.cap.offset) == (0, 8, 16)
    # the outputs drop into dmlc_amd_cuts for to_bins
    h = dm.Cuts
    assert (h.cut_ptr.offset, h.cut_value.offset, h.n_cuts.offset) == (0, 8, 16)
    for s in ("dmlc_amd_make_cuts", "dmlc_amd_make_cuts_workspace_bytes", "dmlc_amd_make_cuts_geometry"):
        assert s in dm.EXPORTED_SYMBOLS and hasattr(dm.lib(), s)
    assert dm.lib().dmlc_amd_abi_version() == 2


def test_geometry_and_workspace_are_sane(dm):
    T, bits = dm.make_cuts_geometry()
    assert T >= 256 and T % 256 == 0 and bits == 8, (T, bits)
    assert dm.lib().dmlc_amd_make_cuts_geometry(None, None) == 0
    _, p, _ = _args(dm)
    ws = lambda m, ncol: dm.lib().dmlc_amd_make_cuts_workspace_bytes(m, ncol, ctypes.byref(p))  # noqa: E731
    assert ws(0, 1) > 0
    # monotone in max_entries; two (column, key) buffers carry the entries
    sizes = [ws(m, 256) for m in (0, 1, T - 1, T, T + 1, 2 * T + 1, 1 << 20, 1 << 24)]
    assert all(b >= a for a, b in zip(sizes, sizes[1:])) and sizes[-1] > sizes[0]
    assert ws(T + 1, 256) > ws(T, 256) >= ws(1, 256)
    assert (1 << 20) * 16 <= ws(1 << 20, 256) <= (1 << 20) * 16 + ((1 << 20) // T + 1) * (256 * 4 + 32) + 16384
    # two words a column
    assert ws(100, 65537) >= ws(100, 256) + (65537 - 256) * 8
    # what the call refuses has no size
    assert ws(100, 0) == 0 and ws((1 << 32) - 1, 256) == 0
    assert ws(100, 1 << 24) == 0 and ws(100, (1 << 24) - 1) > 0  # ncol * max_bin (256) >= 2^32
    assert dm.lib().dmlc_amd_make_cuts_workspace_bytes(100, 256, None) == 0
    for kw in (dict(max_bin=0), dict(index_bits=16), dict(value_type=dm.I32), dict(value_type=dm.I64), dict(flags=1)):
        _, q, _ = _args(dm, **kw)
        assert dm.lib().dmlc_amd_make_cuts_workspace_bytes(100, 256, ctypes.byref(q)) == 0, kw
    _, q, _ = _args(dm)
    q.reserved[1] = 1
    assert dm.lib().dmlc_amd_make_cuts_workspace_bytes(100, 256, ctypes.byref(q)) == 0


def test_a_valid_argument_set_is_what_the_refusals_start_from(dm):
    # (the valid call itself would reach HIP: here only that its workspace has a size)
    _, p, _ = _args(dm)
    assert _ws(dm, p) > 0


def test_null_pointers_are_refused(dm):
    csr, p, c = _args(dm)
    assert _call(dm, None, p, c) == ERR_ARG
    assert _call(dm, csr, None, c) == ERR_ARG
    assert _call(dm, csr, p, None) == ERR_ARG
    assert _call(dm, csr, p, c, res=None) == ERR_ARG
    assert _call(dm, csr, p, c, status=None) == ERR_ARG
    assert _call(dm, csr, p, c, ws=None) == ERR_ARG
    for name in ("cut_ptr", "cut_value"):
        csr, p, c = _args(dm)
        setattr(c, name, None)
        assert _call(dm, csr, p, c) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(ncol=0), dict(max_bin=0), dict(ncol=1 << 24), dict(ncol=1 << 32, max_bin=1),
                                dict(ncol=(1 << 64) - 1), dict(ncol=2, max_bin=1 << 31), dict(ncol=(1 << 32) - 1, max_bin=2),
                                dict(index_bits=16), dict(index_bits=0), dict(value_type=1), dict(value_type=2),
                                dict(value_type=3), dict(value_type=-1), dict(flags=1), dict(flags=8),
                                dict(flags=1 << 31)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_bad_ncol_max_bin_types_and_flags_are_refused(dm, kw):
    csr, p, c = _args(dm, **kw)
    assert _call(dm, csr, p, c, ws_bytes=1 << 40) == ERR_ARG


@pytest.mark.parametrize("word", [0, 1])
def test_a_nonzero_reserved_word_is_refused(dm, word):
    csr, p, c = _args(dm)
    p.reserved[word] = 1
    assert _call(dm, csr, p, c, ws_bytes=1 << 40) == ERR_ARG


@pytest.mark.parametrize("ncol", [1, 256, 257, 65537])
def test_a_small_workspace_is_refused(dm, ncol):
    csr, p, c = _args(dm, ncol=ncol)
    need = _ws(dm, p)
    assert need > 0
    assert _call(dm, csr, p, c, ws_bytes=need - 1) == ERR_ARG
    assert _call(dm, csr, p, c, ws_bytes=0) == ERR_ARG


@pytest.mark.parametrize("out", ["cut_ptr", "cut_value", "status", "ws"])
@pytest.mark.parametrize("src", ["offset", "label", "weight", "qid", "field", "index", "value", "result"])
def test_an_output_that_is_a_source_array_is_refused(dm, out, src):
    csr, p, c = _args(dm)
    ptr = 0x300000 if src == "result" else getattr(csr, src)
    kw = {}
    if out in ("status", "ws"):
        kw[out] = ptr
    else:
        setattr(c, out, ptr)
    assert _call(dm, csr, p, c, **kw) == ERR_ARG


def test_a_window_of_2_to_the_32_rows_or_entries_is_refused(dm):
    big = (1 << 32) - 1
    # rows: min(max_rows, cap[ROWS] - row_begin)
    for cap_rows, row_begin, max_rows in ((big, 0, big), (big + 5, 5, (1 << 64) - 1), (1 << 40, 0, 1 << 33)):
        csr, p, c = _args(dm, row_begin=row_begin, max_rows=max_rows, max_entries=100)
        csr.cap[dm.ROWS] = cap_rows
        assert _call(dm, csr, p, c, ws_bytes=1 << 40) == ERR_ARG
    # entries: max_entries, or cap[INDEX] when it is 0
    for cap_index, max_entries in ((big, 0), (1 << 40, big), (1 << 40, 0), (big + 1, 1 << 50)):
        csr, p, c = _args(dm, max_entries=max_entries)
        csr.cap[dm.INDEX] = cap_index
        assert _call(dm, csr, p, c, ws_bytes=1 << 40) == ERR_ARG
