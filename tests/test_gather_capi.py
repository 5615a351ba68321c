"""CPU-side checks of dmlc_amd_gather_rows's C boundary (no GPU needed): every
argument error is returned before any HIP call, the geometry and the workspace
size are sane and the parameter block has the header's layout."""
import ctypes

import pytest

ERR_ARG = 32


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    dmlc_amd.lib()
    return dmlc_amd


def _csr(dm, base):
    # (never dereferenced: every call below must be refused before any device work)
    c = dm.Csr()
    for i, k in enumerate(("offset", "label", "weight", "qid", "field", "index", "value")):
        setattr(c, k, base + 0x1000 * i)
    for slot in range(7):
        c.cap[slot] = 100
    return c


def _args(dm, **kw):
    p = dm.GatherParams()
    p.index_bits, p.value_type, p.label_type, p.id_bits, p.flags = 32, dm.F32, dm.F32, 64, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return _csr(dm, 0x100000), _csr(dm, 0x200000), p


def _call(dm, src, dst, p, n_ids=10, src_res=0x300000, ids=0x400000, dst_res=0x500000, status=0x600000,
          ws=0x700000, ws_bytes=None):
    if ws_bytes is None:
        ws_bytes = dm.lib().dmlc_amd_gather_workspace_bytes(n_ids)
    ref = lambda x: ctypes.byref(x) if x is not None else None  # noqa: E731
    return dm.lib().dmlc_amd_gather_rows(ref(src), src_res, ids, n_ids, ref(p), ref(dst), dst_res, status, ws,
                                         ws_bytes, None)


def test_gather_params_layout(dm):
    assert ctypes.sizeof(dm.GatherParams) == 32
    f = dm.GatherParams
    assert (f.index_bits.offset, f.value_type.offset, f.label_type.offset, f.id_bits.offset, f.flags.offset,
            f.reserved.offset) == (0, 4, 8, 12, 16, 20)


def test_geometry_and_workspace_are_sane(dm):
    R = dm.gather_geometry()
    assert R >= 256 and R & (R - 1) == 0, R
    assert dm.lib().dmlc_amd_gather_geometry(None) == 0
    ws = dm.lib().dmlc_amd_gather_workspace_bytes
    assert ws(0) > 0 and ws(1) >= ws(0) and ws(R + 1) >= ws(R)
    # a few words per tile, not per id
    assert ws(1 << 30) <= (1 << 30) // R * 64 + 4096
    assert ws(1 << 30) > ws(1 << 20) > ws(1)


def test_null_pointers_are_refused(dm):
    src, dst, p = _args(dm)
    assert _call(dm, None, dst, p) == ERR_ARG
    assert _call(dm, src, None, p) == ERR_ARG
    assert _call(dm, src, dst, None) == ERR_ARG
    assert _call(dm, src, dst, p, src_res=None) == ERR_ARG
    assert _call(dm, src, dst, p, dst_res=None) == ERR_ARG
    assert _call(dm, src, dst, p, status=None) == ERR_ARG
    assert _call(dm, src, dst, p, ws=None) == ERR_ARG
    assert _call(dm, src, dst, p, ids=None) == ERR_ARG  # ids to read but no array
    dst.offset = None  # dst.offset[0] is always written
    assert _call(dm, src, dst, p) == ERR_ARG
    assert _call(dm, src, dst, p, n_ids=0, ids=None) == ERR_ARG


@pytest.mark.parametrize("kw", [dict(index_bits=16), dict(index_bits=0), dict(value_type=3), dict(value_type=-1),
                                dict(label_type=3), dict(label_type=-1), dict(id_bits=16), dict(id_bits=0),
                                dict(id_bits=-64), dict(flags=1), dict(flags=2), dict(flags=4), dict(flags=16),
                                dict(flags=8 | 1), dict(flags=1 << 31)],
                         ids=lambda kw: ",".join("%s=%s" % kv for kv in kw.items()))
def test_bad_types_and_flags_are_refused(dm, kw):
    src, dst, p = _args(dm, **kw)
    assert _call(dm, src, dst, p) == ERR_ARG


@pytest.mark.parametrize("word", [0, 1, 2])
def test_a_nonzero_reserved_word_is_refused(dm, word):
    src, dst, p = _args(dm)
    p.reserved[word] = 1
    assert _call(dm, src, dst, p) == ERR_ARG


def test_a_small_workspace_is_refused(dm):
    R = dm.gather_geometry()
    src, dst, p = _args(dm)
    for n in (0, 1, R, 100 * R + 1):
        need = dm.lib().dmlc_amd_gather_workspace_bytes(n)
        assert _call(dm, src, dst, p, n_ids=n, ws_bytes=need - 1) == ERR_ARG
    assert _call(dm, src, dst, p, n_ids=10, ws_bytes=0) == ERR_ARG


def test_more_tiles_than_a_launch_holds_is_refused_not_truncated(dm):
    R = dm.gather_geometry()
    limit = (1 << 31) - 1
    src, dst, p = _args(dm)
    for n in (limit * R + 1, (limit + 1) * R, 1 << 62, (1 << 64) - 1):
        assert _call(dm, src, dst, p, n_ids=n, ws_bytes=1 << 62) == ERR_ARG


@pytest.mark.parametrize("name", ["offset", "label", "weight", "qid", "field", "index", "value"])
def test_a_dst_array_that_is_the_src_array_is_refused(dm, name):
    src, dst, p = _args(dm)
    setattr(dst, name, getattr(src, name))
    assert _call(dm, src, dst, p) == ERR_ARG


def test_a_dst_result_block_that_is_the_src_block_is_refused(dm):
    src, dst, p = _args(dm)
    assert _call(dm, src, dst, p, src_res=0x300000, dst_res=0x300000) == ERR_ARG
