"""GPU parity of the ONE-CALL parse pipeline (dmlc_amd_parse with flags = 0:
what the host engine behind dmlc::Parser and bench.py run) against the oracle.

The other GPU parity files go through dmlc_amd.parse_bytes: COUNT_ONLY, an
allocation of the exact counts, FILL_ONLY.  Here every parse is one call into
outputs whose capacities are not the exact counts (tests/full_call.py): the
hand-over from the single-pass kernel to the exact kernels inside the call
after earlier tiles have stored their rows, capacities above and below the
counts, one parser / workspace / result block reused over many calls, and the
lean libsvm kernel (svm_lean.h, DMLC_AMD_LEAN=1), which only a full call
launches.  Arrays, counts and the unit table are compared bit for bit, and a
guard band behind every capacity must stay untouched.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import full_call as fc
from golden_util import load_json
from oracle import pyoracle as po
from tools import synth

pytestmark = pytest.mark.gpu

FMTS = [po.LIBSVM, po.CSV, po.LIBFM]
IDS = ["libsvm", "csv", "libfm"]


@pytest.fixture(scope="module")
def dm():
    import dmlc_amd
    import torch
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    dmlc_amd.lib()
    return dmlc_amd


def _oracle(dm, data, offs, fmt, kw):
    prm = dm.make_params(fc.FMT_NAME[fmt], **kw)
    return prm, po.parse_chunks(data, offs, fmt=fmt, **fc.oracle_kw(prm))


# ------------------------------------------------ a. differential fuzz --
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_gpu_full_call_fuzz_vs_oracle(dm, fmt):
    """Every input of full_call.*_cases (half single-tile, half 4-12 tiles;
    clean, violating and placed-violation classes, chunk cuts at line ends and
    anywhere, indexing modes, id widths, nthread 1-3) through one full call
    with capacities of the exact counts + 0, + 1 and + 1000, some with the
    engine's bound len / 2 + 2 in every slot, and once with FLAG_EXACT.  Inputs
    clean by construction must stay on the single pass (path == 0), a placed
    violation must hand over inside the call, FLAG_EXACT must report the
    exact kernels."""
    tile = dm.fast_geometry()[0]
    cases = fc.CASES[fmt](tile)
    stay = hand = compared = 0
    for c in cases:
        data, offs, kw = c["data"], c["offs"], c["kw"]
        try:
            prm, o = _oracle(dm, data, offs, fmt, kw)
            assert o["status"] == 0 or not c["parsed"], o["msg"]  # an input built for the array comparison
            compared += o["status"] == 0
            split = fc.split_table(dm, data, offs, prm) if o["status"] == 0 else None
            paths = set()
            for slack in (0, 1, 1000):
                h = fc.full_vs_oracle(dm, data, offs, fmt, oracle=o, split=split, slack=slack, **kw)
                paths.add(h["path"])
            if c["name"].startswith(("multi0", "placed_", "base_")) and o["status"] == 0:
                h = fc.full_vs_oracle(dm, data, offs, fmt, oracle=o, split=split, caps=[len(data) // 2 + 2] * 7, **kw)
                paths.add(h["path"])
            assert len(paths) == 1, paths  # the capacities do not steer the path
            he = fc.full_vs_oracle(dm, data, offs, fmt, oracle=o, split=split, exact=True, **kw)
            assert he["path"] != 0
            path = paths.pop()
            if c["expect"] == "stay":
                assert path == 0, path
            if c["expect"] == "hand":
                assert path != 0, path
        except AssertionError as e:
            raise AssertionError("%s kw=%s offs=%s: %s" % (c["name"], kw, offs[:12], e))
        stay += path == 0
        hand += path != 0
    print("full-call fuzz %s: %d inputs, %d stayed single-pass, %d handed over; arrays compared for %d, failure status for %d"
          % (IDS[FMTS.index(fmt)], len(cases), stay, hand, compared, len(cases) - compared))
    assert 3 * stay >= len(cases) and 5 * hand >= len(cases), (len(cases), stay, hand)
    assert 3 * compared >= 2 * len(cases), (len(cases), compared)


# ---------------------------------------------- b. genuine-reference pin --
def _sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


@pytest.mark.parametrize("name", ["libsvm_10k_x128", "csv_10k_x256"])
def test_gpu_full_call_synthetic_config1(dm, name):
    """BASELINE config 1 (generated and chunked as test_gpu_synthetic_config1
    does) through one full call with 1000 spare elements per slot: every
    array, trimmed to its count, hashes to what the genuine reference gave."""
    g = load_json("synth_cfg1.json")[name]
    fmt = po.LIBSVM if g["format"] == "libsvm" else po.CSV
    text, _ = synth.rows(synth.LIBSVM if fmt == po.LIBSVM else synth.CSV, g["rows"], g["width"], seed=g["seed"])
    assert _sha(text) == g["input_sha256"]
    chunks = po.split_text([text.tobytes()])
    offs = np.cumsum([0] + [len(c) for c in chunks]).tolist()
    h = fc.full_vs_oracle(dm, b"".join(chunks), offs, fmt, slack=1000)
    assert h["error"] == 0 and h["path"] == 0
    for k, hv in g["sha256"].items():
        assert _sha(h[k]) == hv, k


# ------------------------------------------------- c. capacity contract --
CAP_PARAMS = [(f, m, im) for f in FMTS for m in ("stay", "hand", "exact") for im in ((0,) if f == po.CSV else (0, -1))]


@pytest.mark.parametrize("fmt,mode,im", CAP_PARAMS,
                         ids=["%s-%s-im%d" % (IDS[FMTS.index(f)], m, im) for f, m, im in CAP_PARAMS])
def test_gpu_full_call_capacity_contract(dm, fmt, mode, im):
    """dmlc_amd.h: an output too small gives ERR_CAPACITY with exact counts.
    A three-tile input that stays on the single pass, one that hands over
    inside the call and one under FLAG_EXACT, with each slot the format has
    under-sized alone (count - 1, count / 2, 0) and two at once: the error,
    the counts, nothing written at or past a capacity; then the engine's
    retry on the same parser and result block with the reported counts, equal
    to the oracle.  (Labels of libsvm / libfm go by cap[ROWS]: LABEL is a CSV
    slot.)"""
    import torch
    tile = dm.fast_geometry()[0]
    data, offs, kw = fc.capacity_input(fmt, mode, tile)
    if fmt != po.CSV:
        kw["indexing_mode"] = im
    parser = fc.make_parser(dm, fmt, kw)
    res = torch.zeros(16, dtype=torch.int64, device="cuda")
    o = po.parse_chunks(data, offs, fmt=fmt, **fc.oracle_kw(parser.params))
    assert o["status"] == 0, o["msg"]
    h = fc.full_vs_oracle(dm, data, offs, fmt, parser=parser, result=res, oracle=o)
    assert (h["path"] == 0) == (mode == "stay"), h["path"]
    counts = fc.oracle_counts(o)
    own = {po.LIBSVM: [fc.WEIGHT, fc.QID], po.CSV: [fc.WEIGHT, fc.LABEL], po.LIBFM: [fc.WEIGHT, fc.FIELD]}[fmt]
    slots = [fc.ROWS, fc.INDEX, fc.VALUE] + own
    assert all(counts[s] > 1 for s in slots), counts
    for s in slots:
        for c in (counts[s] - 1, counts[s] // 2, 0):
            caps = list(counts)
            caps[s] = c
            fc.under_sized(dm, data, offs, fmt, caps, parser, res, o)
    for a, b in ((fc.INDEX, fc.VALUE), (fc.ROWS, own[1]), (own[0], fc.INDEX)):
        caps = list(counts)
        caps[a], caps[b] = counts[a] // 2, counts[b] - 1
        fc.under_sized(dm, data, offs, fmt, caps, parser, res, o)


# ------------------------------------ d. one parser reused across calls --
def _reuse_sequence(fmt, tile):
    """[(name, data, offs, slack or None for the under-sized call)]"""
    rng = np.random.default_rng(4100 + fmt)
    ft, sized, lf = fc.fuzz_text, fc.grown, fc.lf
    V = lambda g: fc.valued(g, fmt)  # noqa: E731
    cut = lambda d, n=5: ft.random_cuts(rng, d, n)  # noqa: E731
    if fmt == po.LIBSVM:
        clean = lambda nb: sized(V(lambda n: ft.uniform_libsvm(rng, n, 12)), nb)  # noqa: E731
        qbase = lf(sized(V(lambda n: ft.qid_libsvm(rng, n, 40)), 6 * tile + 999))
        small_bad, bad_line, err = b"1 2:3 3:\n0 1:1\n2 5:6 # c\n", b"1 2:3 4:5", b"1 -3:1\n"
        rows7 = sized(V(lambda n: ft.qid_libsvm(rng, n, 30)), 5 * tile)
        rows8 = sized(V(lambda n: ft.qid_libsvm(rng, n, 30, mixed=True)), 4 * tile + 77)
        vbase = qbase
    elif fmt == po.CSV:
        clean = lambda nb: sized(lambda n: ft.labeled_csv(rng, n, 12, 0, weight_col=2), nb)  # noqa: E731
        small_bad, bad_line, err = b"1,2,3,4\n0,5,6, \n1,6,7,8\n", fc.blank_last(12), b"1,2,3\n7\n"
        rows7 = sized(lambda n: ft.labeled_csv(rng, n, 30, 0, weight_col=2), 5 * tile).replace(b"\n", b"\r\n")
        rows8 = sized(lambda n: ft.labeled_csv(rng, n, 9, 0, defects=0.1, weight_col=2), 4 * tile + 77)
        vbase = clean(6 * tile + 999)
    else:
        clean = lambda nb: sized(lambda n: ft.libfm_rows(rng, n, 20), nb)  # noqa: E731
        small_bad, bad_line, err = b"1 1:2:3:4\n0 2:3:4\n", b"1 1:2:3:4", b"1 -3:4:5\n"
        rows7 = sized(lambda n: ft.libfm_rows(rng, n, 9, weights=True), 5 * tile)
        rows8 = sized(lambda n: ft.uniform_libfm(rng, n, 8, violate=True), 4 * tile + 77)
        vbase = clean(6 * tile + 999)
    big, less = clean(8 * tile + 321), clean(3 * tile + 5)
    nt = (len(vbase) + tile - 1) // tile
    last, empty = fc.place_violation(vbase, bad_line, nt - 1, tile)
    early = fc.empty_line_cut(last, 0, (nt - 1) * tile) if fmt == po.LIBSVM else ()  # (the other generators draw no empty lines)
    assert early or fmt != po.LIBSVM
    return [("large_clean", big, cut(big), 1000), ("small_violating", small_bad, [0, len(small_bad)], 1000),
            ("violation_in_last_tile", last, fc.with_cuts(cut(last), empty + early), 1000), ("empty", b"", [0], 1000),
            ("reference_error", err, [0, len(err)], 1000), ("fewer_tiles", less, cut(less), 1000),
            ("rows7", rows7, cut(rows7), 1), ("rows8", rows8, cut(rows8), 1000), ("large_clean_again", big, cut(big), 1),
            ("slack0", less, cut(less), 0), ("under_sized", big, cut(big), None), ("clean_after_error", less, cut(less), 1000)]


@pytest.mark.parametrize("fill", [0xFF, 0], ids=["ws_ff", "ws_zero"])
@pytest.mark.parametrize("fmt", FMTS, ids=IDS)
def test_gpu_full_call_reuse(dm, fmt, fill):
    """One DeviceParser, one workspace (all 0xFF or all zero before the first
    call: dmlc_amd.h asks for no zeroing), one result block and one output
    set over twelve full calls and the retry of the under-sized one -- large
    clean, small violating, a violation in the last tile, empty, a reference
    error, fewer tiles, qid on every row (CSV: CRLF rows, libfm: weights), a
    mix, clean again, exact capacities, ERR_CAPACITY, clean -- each compared
    with the oracle before the next starts: nothing of a call (look-back
    words, gates, qid sums, unit minima, error word) leaks into the next."""
    import torch
    tile = dm.fast_geometry()[0]
    seq = _reuse_sequence(fmt, tile)
    # MAX_INDEX as the host engine calls it; three ParseBlock ranges per chunk, so the one-byte chunks
    # of the placed violation hold units without a line, whose table rows only the finish kernel fills
    kw = {"flags": fc.FLAG_MAX_INDEX, "nthread": 3}
    if fmt == po.CSV:
        kw.update(label_column=0, weight_column=2)
    parser = fc.make_parser(dm, fmt, kw)
    prm = parser.params
    need = max(dm.lib().dmlc_amd_workspace_bytes(len(d), max(len(offs) - 1, 1), ctypes.byref(prm)) for _, d, offs, _ in seq)
    ws = torch.full((need,), fill, dtype=torch.uint8, device="cuda")
    parser._ws = ws
    big = max(len(d) for _, d, _, _ in seq)
    outs = fc.new_outputs(prm, {k: big + 2 + 1000 for k in fc.ARRAYS})  # (len + 2 per slot when the oracle raises)
    res = torch.zeros(16, dtype=torch.int64, device="cuda")
    assert len(seq) >= 12
    for name, data, offs, slack in seq:
        try:
            o = po.parse_chunks(data, offs, fmt=fmt, **fc.oracle_kw(prm))
            if slack is None:
                assert o["status"] == 0
                caps = fc.oracle_counts(o)
                caps[fc.INDEX] //= 2
                h = fc.parse_full(dm, data, offs, fmt, caps=caps, parser=parser, result=res, outputs=outs)
                assert dm.error_code(h["error"]) == dm.ERR_CAPACITY and h["counts"][:7] == fc.oracle_counts(o)
                fc.full_vs_oracle(dm, data, offs, fmt, parser=parser, result=res, outputs=outs, oracle=o, caps=h["counts"][:7])
            else:
                fc.full_vs_oracle(dm, data, offs, fmt, parser=parser, result=res, outputs=outs, oracle=o, slack=slack)
        except AssertionError as e:
            raise AssertionError("call %s: %s" % (name, e))
    assert parser._ws is ws  # the same workspace served every call


# ------------------------------------------------------ e. lean kernel --
def test_gpu_lean_kernel_full_call_vs_oracle(dm):
    """svm_lean_tile launches only in a full call with DMLC_AMD_LEAN=1, read
    once when the library loads: a child process (tests/lean_child.py) sets it,
    loads the product library and compares full calls with the oracle.  The
    clustered many-chunks input (more unit starts in one tile than
    svm_fast_tile takes) stays on the single pass only when the lean kernel
    ran: path == 0 in the child, path != 0 here without the variable."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tests", "lean_child.py")], capture_output=True, timeout=240)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert [c for c in out["cases"] if not c["ok"]] == []
    assert all(c["status"] == 0 for c in out["cases"] if c["parsed"]), [c["name"] for c in out["cases"] if c["status"]]
    for c in out["cases"]:
        if c["expect"] == "stay":
            assert c["path"] == 0, c
        if c["expect"] == "hand":
            assert c["path"] != 0, c
    stay = sum(c["path"] == 0 for c in out["cases"])
    print("lean child: %d inputs, %d stayed single-pass, %d handed over; arrays compared for %d"
          % (len(out["cases"]), stay, len(out["cases"]) - stay, sum(c["status"] == 0 for c in out["cases"])))
    assert len(out["cases"]) >= 16
    assert out["cluster_path"] == 0, out["cluster_path"]
    tile, max_cs = dm.fast_geometry()
    data, offs = fc.cluster_chunks(tile, max_cs)
    h = fc.full_vs_oracle(dm, data, offs, po.LIBSVM)
    assert h["path"] != 0, h["path"]
