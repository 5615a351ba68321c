"""CPU checks of the one-call GPU tests' inputs (tests/test_gpu_full_call.py):
every input of full_call.*_cases and full_call.lean_cases whose path is fixed
by construction, and the lean kernel's cluster input, through the emulator --
so that "stays on the single pass" / "hands over" is verified where no GPU is
present.  (The emulator reports the path the GPU call reports.)"""
import pytest

import full_call as fc
from golden_util import diff
from oracle import pyoracle as po
from tests.emu import pyemu, pyemu_ws

EMU_MAX = 400000  # bytes: the 1.4 MB wide-rows input of the lean cases takes the emulator too long


def _failed(h, name, offs, nthread=1):
    import dmlc_amd
    nunits = (len(offs) - 1) * max(nthread, 1)
    return bool(h["error"]) or (nunits > 0 and dmlc_amd.chunk_check(h, name, nunits, h["counts"]) >= 0)


@pytest.mark.parametrize("which", ["libsvm", "csv", "libfm", "lean"])
def test_emu_full_call_input_classes(which, monkeypatch):
    """Every placed violation -- one violating line in the first, a middle and
    the last tile of clean text -- hands over to the exact kernels; the clean
    base texts and the single- and multi-tile inputs of the clean generator
    classes stay on the single pass ("lean": the lean child's inputs with
    DMLC_AMD_LEAN=1); each equals the oracle, and the inputs built for the
    array comparison are parsed by it."""
    import dmlc_amd
    tile = dmlc_amd.fast_geometry()[0]
    if which == "lean":
        monkeypatch.setenv("DMLC_AMD_LEAN", "1")
        fmt, cases = po.LIBSVM, fc.lean_cases(tile)
    else:
        monkeypatch.delenv("DMLC_AMD_LEAN", raising=False)
        fmt = {"libsvm": po.LIBSVM, "csv": po.CSV, "libfm": po.LIBFM}[which]
        cases = fc.CASES[fmt](tile)
    name = fc.FMT_NAME[fmt]
    seen = {"stay": 0, "hand": 0}
    for c in cases:
        data, offs = c["data"], c["offs"]
        kw = {k: v for k, v in c["kw"].items() if k != "flags"}
        okw = {("value_kind" if k == "value_type" else k): v for k, v in kw.items()}
        o = po.parse_chunks(data, offs, fmt=fmt, **okw)
        assert o["status"] == 0 or not c["parsed"], (c["name"], o["msg"])
        if not c["expect"] or len(data) > EMU_MAX:
            continue
        if c["name"].startswith("placed_"):
            t = int(c["name"].rsplit("_t", 1)[1])
            a = offs[[i for i in range(len(offs) - 1) if offs[i + 1] - offs[i] == 1 and data[offs[i]:offs[i + 1]] == b"\n"][-1]]
            assert t * tile < a < (t + 1) * tile, (c["name"], a)  # the placed line lies in its tile
        h = pyemu_ws.parse(data, offs, **kw) if fmt == po.CSV else pyemu.parse(data, offs, name, **kw)
        failed = _failed(h, name, offs, kw.get("nthread", 1))
        assert (o["status"] != 0) == failed, (c["name"], o["msg"], h["error"])
        if not failed:
            assert diff(h, o) == [], (c["name"], diff(h, o))
        assert h["path"] == ("fast" if c["expect"] == "stay" else "exact"), (c["name"], kw, h["path"])
        seen[c["expect"]] += 1
    assert seen["hand"] >= 3 and seen["stay"] >= 6, seen


@pytest.mark.parametrize("lean,want", [("1", "fast"), ("0", "exact")])
def test_emu_full_call_lean_cluster(lean, want, monkeypatch):
    """The bytes and chunk starts the lean-kernel GPU test proves the launch
    with (full_call.cluster_chunks): on the single pass with DMLC_AMD_LEAN=1,
    on the exact kernels without it."""
    import dmlc_amd
    tile, max_cs = dmlc_amd.fast_geometry()
    data, offs = fc.cluster_chunks(tile, max_cs)
    o = po.parse_chunks(data, offs, fmt=po.LIBSVM)
    monkeypatch.setenv("DMLC_AMD_LEAN", lean)
    h = pyemu.parse(data, offs, "libsvm")
    assert o["status"] == 0 and not _failed(h, "libsvm", offs)
    assert diff(h, o) == [] and h["path"] == want, (lean, h["path"])
