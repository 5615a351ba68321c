"""TEST INFRASTRUCTURE ONLY -- child process of tests/test_gpu_graph.py.

include/dmlc_amd.h promises that no call synchronises, allocates or runs a
device-wide barrier, "so calls can be captured into a hipGraph".  This process
captures the calls with torch.cuda.graph in its default (global) error mode --
an allocation or a synchronisation inside a call fails the capture -- on ONE
stream as a linear sequence, and replays the graph over device data that
changes between replays: the next member of a replay family
(tests/graph_cases.py) is copied into the same device tensors, every output is
refilled with its sentinel, and the workspaces stay as the previous replay left
them (poisoned with 0xCD once, before the first replay).  Each replay is
compared bit for bit with the oracle (parse) or the numpy models over the
oracle's CSR (post-parse calls).

    graph_child.py parse:<configuration> | back_to_back | copy_out | copy | chain | two_graphs

One process per test, so that a failed capture leaves no broken stream state
behind.  Prints one JSON line: {"ok", "msg", "order", "paths", ...}.
"""
import ctypes
import json
import os
import sys
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
os.environ.pop("DMLC_AMD_LIB", None)  # the product library, not a variant
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "dmlc-core_amd", "python")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import dmlc_amd as dm  # noqa: E402
import full_call as fc  # noqa: E402
import graph_cases as gc  # noqa: E402
from golden_util import diff  # noqa: E402
from oracle import pyoracle as po  # noqa: E402

U8 = torch.uint8
WS_POISON = 0xCD


def geometry():
    return {"csc": dm.csc_geometry()[0], "cuts": dm.make_cuts_geometry()[0], "gather": dm.gather_geometry(),
            "dense": dm.dense_geometry(), "bins": dm.bins_geometry()}


def dev_bytes(raw):
    return torch.frombuffer(bytearray(raw), dtype=U8)


def capture(fn):
    """fn() captured on torch.cuda.graph's own capture stream, error mode "global"."""
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


class ParseRig:
    """Everything one captured dmlc_amd_parse call holds on to: device text and
    chunk starts of a fixed size, sentinel-guarded outputs of fixed capacities
    (full_call.new_outputs), the unit table and the result block."""

    def __init__(self, fmt, kw, nbytes, nchunks, caps, parser=None):
        self.parser = parser if parser is not None else fc.make_parser(dm, fmt, kw)
        prm = self.prm = self.parser.params
        self.caps = [int(c) for c in caps[:7]]
        self.acap = fc.array_caps(prm, self.caps)
        self.dt = fc._dtypes(prm)
        self.outs = fc.new_outputs(prm, self.acap)
        self.text = torch.empty(nbytes, dtype=U8, device="cuda")
        self.cs = torch.empty(nchunks + 1, dtype=torch.int64, device="cuda")
        self.nchunks = nchunks
        self.upc = dm.units_per_chunk(prm)
        self.nunits = nchunks * self.upc
        self.tab = torch.empty((self.nunits * 8 + fc.GUARD) * 8, dtype=U8, device="cuda")
        self.tab64 = self.tab.view(torch.int64)
        self.res = torch.zeros(16, dtype=torch.int64, device="cuda")
        self.csr = dm.Csr()
        for k in fc.ARRAYS:
            setattr(self.csr, k, self.outs[k].data_ptr())
        for i, c in enumerate(self.caps):
            self.csr.cap[i] = c
        self.arg = {"_csr": self.csr}

    def load(self, member):
        assert len(member["data"]) == self.text.numel() and len(member["offs"]) == self.cs.numel()
        self.text.copy_(dev_bytes(member["data"]))
        self.cs.copy_(torch.tensor(member["offs"], dtype=torch.int64))

    def refill(self):
        for k in fc.ARRAYS:
            self.outs[k].fill_(fc.SENT_BYTE)
        self.tab.fill_(fc.SENT_BYTE)
        self.tab[:self.nunits * 64].zero_()  # as DeviceParser.parse hands it over

    def call(self):
        self.parser.parse_into(self.text, self.cs, self.arg, self.res, chunk_table=self.tab64)

    def collect(self):
        """full_call.parse_full's read-back: the arrays trimmed to min(count,
        capacity), the guard bands asserted, and "raw": every byte of every
        output and result words 0 - 11."""
        torch.cuda.synchronize()
        r = self.res.cpu().numpy().view(np.uint64)
        counts = [int(x) for x in r[:8]]
        cnt = fc.array_caps(self.prm, counts)
        h, touched, raw = {}, [], {}
        for k in fc.ARRAYS:
            b = self.outs[k].cpu().numpy()
            isz = np.dtype(self.dt[k]).itemsize
            if not (b[self.acap[k] * isz:] == fc.SENT_BYTE).all():
                touched.append(k)
            h[k] = b[:min(cnt[k], self.acap[k]) * isz].view(self.dt[k])
            raw[k] = b.tobytes()
        tb = self.tab.cpu().numpy()
        if not (tb[self.nunits * 64:] == fc.SENT_BYTE).all():
            touched.append("chunk_table")
        assert touched == [], ("written at or past the capacity", touched, self.caps, counts)
        raw["chunk_table"] = tb.tobytes()
        raw["result"] = r[:12].tobytes()
        h["chunk_table"] = tb[:self.nunits * 64].view(np.uint64).reshape(-1, 8)
        h.update(counts=counts, error=int(r[8]), path=int(r[9]), max_index=int(r[10]), max_field=int(r[11]),
                 units_per_chunk=self.upc, caps=self.caps, raw=raw)
        return h

    def poison_workspace(self):
        self.parser._ws.fill_(WS_POISON)


def check_parse(rig, h, member, o, split=None):
    """full_call.full_vs_oracle's assertions for one replay, by the member's
    label: the failure status (D: the error word; E: ERR_CAPACITY with exact
    counts), the counts, every array, the unit table, max_index / max_field
    and the path."""
    name = fc.FMT_NAME[fc._fmt_of(rig.prm)]
    expect = member["expect"]
    if expect == "capacity":
        assert o["status"] == 0 and dm.error_code(h["error"]) == dm.ERR_CAPACITY, (h["error"], h["counts"], rig.caps)
        assert h["counts"][:7] == fc.oracle_counts(o), (h["counts"], fc.oracle_counts(o))
        return
    failed = bool(h["error"]) or dm.chunk_check(h, name, rig.nunits, h["counts"]) >= 0
    assert (o["status"] != 0) == failed, (o["msg"], h["error"], h["path"])
    if expect == "error":
        code, pos = member["err"]
        assert failed and h["error"] == (pos << 16) | code, (dm.error_pos(h["error"]), dm.error_code(h["error"]), pos, code)
        return
    assert h["counts"][:7] == fc.oracle_counts(o), (h["counts"], fc.oracle_counts(o), h["path"])
    bad = diff(h, o)
    assert bad == [], (bad, h["path"])
    if split is not None:
        assert h["chunk_table"].tolist() == np.asarray(split).tolist(), ("unit table", h["path"])
    if rig.prm.flags & fc.FLAG_MAX_INDEX:
        for key, got in (("index", h["max_index"]), ("field", h["max_field"])):
            if len(o[key]):
                assert got == int(np.asarray(o[key]).max()), (key, got)
    if rig.prm.flags & fc.FLAG_EXACT:
        assert h["path"] != 0, h["path"]
    elif expect == "stay":
        assert h["path"] == 0, h["path"]
    elif expect == "hand":
        assert h["path"] != 0, h["path"]


def same_raw(a, b, what):
    bad = [k for k in a if a[k] != b[k]]
    assert bad == [], (what, bad)


def parse_setup(config):
    tile = dm.fast_geometry()[0]
    name, kw = gc.config_kw(config)
    fam = gc.family(name, tile)
    M = fam["members"]
    o = {m: gc.oracle_of(fam, m, kw) for m in M}
    rig = ParseRig(fam["fmt"], kw, fam["nbytes"], fam["nchunks"], gc.captured_caps(o))
    split = {m: fc.split_table(dm, M[m]["data"], M[m]["offs"], rig.prm) for m in "ABC"}
    return fam, M, o, rig, split


def eager_then_capture(rig, member, o, split, extra=None):
    """The call once eagerly on the rig's buffers (code objects loaded, the
    parser's workspace grown), compared with the oracle; then the capture; then
    the workspace poisoned.  -> (graph, the eager read-back)."""
    rig.load(member)
    rig.refill()
    rig.call()
    if extra:
        extra()
    eager = rig.collect()
    check_parse(rig, eager, member, o, split)
    ws = rig.parser._ws

    def calls():
        rig.call()
        if extra:
            extra()
    g = capture(calls)
    assert rig.parser._ws is ws  # no workspace was allocated under the capture
    rig.poison_workspace()
    return g, eager


def run_parse(config):
    """One graph, replayed A, B, C, A, D, A, E, A."""
    fam, M, o, rig, split = parse_setup(config)
    g, eager = eager_then_capture(rig, M["A"], o["A"], split["A"])
    paths, errors = [], []
    for i, m in enumerate(gc.ORDER):
        rig.load(M[m])
        rig.refill()
        g.replay()
        h = rig.collect()
        try:
            check_parse(rig, h, M[m], o[m], split.get(m))
            if m == "A":  # byte-identical to the eager call, so to every other replay of A
                same_raw(h["raw"], eager["raw"], "A replayed vs eager")
        except AssertionError as e:
            raise AssertionError("replay %d (%s): %s" % (i, m, e))
        paths.append(h["path"])
        errors.append(dm.error_code(h["error"]))
    return {"order": list(gc.ORDER), "paths": paths, "errors": errors, "nbytes": fam["nbytes"],
            "nchunks": fam["nchunks"], "units": rig.nunits, "caps": rig.caps}


def run_back_to_back():
    """A's graph launched twice with no host work in between, then one synchronise."""
    fam, M, o, rig, split = parse_setup("libfm_max_index")
    g, eager = eager_then_capture(rig, M["A"], o["A"], split["A"])
    rig.load(M["A"])
    rig.refill()
    g.replay()
    g.replay()
    h = rig.collect()
    check_parse(rig, h, M["A"], o["A"], split["A"])
    same_raw(h["raw"], eager["raw"], "A twice vs eager")
    return {"order": ["A", "A"], "paths": [h["path"]]}


# the engine's copy-out (host/hip_engine.h): the CSR arrays and the unit table by dmlc_amd_copy_n_dev, sizes read on
# the device from the parse's result block
COPY_NAMES = ("offset", "label", "weight", "qid", "index", "field", "value", "chunk_table")
COPY_SLOT = (fc.ROWS, fc.LABEL, fc.WEIGHT, fc.QID, fc.INDEX, fc.FIELD, fc.VALUE, -1)
HOST_TAIL = 64


def _copy_n_dev():
    L = dm.lib()
    f = L.dmlc_amd_copy_n_dev
    f.restype = ctypes.c_int
    P = ctypes.POINTER
    f.argtypes = [P(ctypes.c_void_p), P(ctypes.c_void_p), ctypes.c_void_p, P(ctypes.c_int), P(ctypes.c_uint64),
                  P(ctypes.c_uint64), P(ctypes.c_uint64), ctypes.c_int, ctypes.c_void_p]
    return f


def run_copy_out():
    """parse_into, then dmlc_amd_copy_n_dev into page-locked host arrays, in one graph: A, then B."""
    fam, M, o, rig, split = parse_setup("csv_max_index")
    copy_n_dev = _copy_n_dev()
    isz = {k: np.dtype(rig.dt[k]).itemsize for k in fc.ARRAYS}
    scale = [isz[k] if k != "chunk_table" else 0 for k in COPY_NAMES]
    add = [8] + [0] * 6 + [rig.nunits * 64]
    maxb = [rig.acap[k] * isz[k] if k != "chunk_table" else rig.nunits * 64 for k in COPY_NAMES]
    host = [torch.empty(n + HOST_TAIL, dtype=U8).pin_memory() for n in maxb]
    src = [rig.outs[k].data_ptr() if k != "chunk_table" else rig.tab.data_ptr() for k in COPY_NAMES]
    n = len(COPY_NAMES)
    a_dst = (ctypes.c_void_p * n)(*[t.data_ptr() for t in host])
    a_src = (ctypes.c_void_p * n)(*src)
    a_slot = (ctypes.c_int * n)(*COPY_SLOT)
    a_scale, a_add, a_max = ((ctypes.c_uint64 * n)(*v) for v in (scale, add, maxb))

    def copy_out():
        rc = copy_n_dev(a_dst, a_src, rig.res.data_ptr(), a_slot, a_scale, a_add, a_max, n,
                        torch.cuda.current_stream().cuda_stream)
        assert rc == 0, rc
    g, _ = eager_then_capture(rig, M["A"], o["A"], split["A"], extra=copy_out)
    paths = []
    for m in ("A", "B"):
        rig.load(M[m])
        rig.refill()
        for t in host:
            t.fill_(fc.SENT_BYTE)
        g.replay()
        h = rig.collect()
        check_parse(rig, h, M[m], o[m], split[m])
        paths.append(h["path"])
        for k, t in zip(COPY_NAMES, host):
            want = np.asarray(split[m], dtype=np.uint64).tobytes() if k == "chunk_table" else \
                np.asarray(o[m][k]).astype(rig.dt[k]).tobytes()
            got = t.numpy().tobytes()
            assert len(want) + HOST_TAIL <= len(got), (k, len(want), len(got))
            assert got[:len(want)] == want, (m, k, "the host array differs from the oracle")
            assert got[len(want):] == bytes([fc.SENT_BYTE]) * (len(got) - len(want)), (m, k, "sentinel tail written")
    return {"order": ["A", "B"], "paths": paths}


def run_copy():
    """One aligned and one unaligned dmlc_amd_copy (device to device) of a few
    KiB plus 15 bytes, each in a graph of its own, each replayed twice over
    changed source bytes."""
    L = dm.lib()
    n, lead = 5 * 1024 + 15, 16
    rng = np.random.default_rng(6)
    out = {}
    for name, shift in (("aligned", 0), ("unaligned", 1)):
        src = torch.zeros(n + 32, dtype=U8, device="cuda")
        dst = torch.empty(n + 2 * lead, dtype=U8, device="cuda")
        assert (src.data_ptr() | dst.data_ptr()) & 15 == 0

        def call():
            rc = L.dmlc_amd_copy(dst.data_ptr() + lead, src.data_ptr() + shift, n, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
        call()
        torch.cuda.synchronize()
        g = capture(call)
        for rep in range(2):
            data = rng.integers(0, 256, size=n + 32, dtype=np.uint8)
            src.copy_(torch.from_numpy(data))
            dst.fill_(fc.SENT_BYTE)
            g.replay()
            torch.cuda.synchronize()
            got = dst.cpu().numpy()
            assert got[lead:lead + n].tobytes() == data[shift:shift + n].tobytes(), (name, rep)
            assert (got[:lead] == fc.SENT_BYTE).all() and (got[lead + n:] == fc.SENT_BYTE).all(), (name, rep, "guard")
        out[name] = 2
    return {"replays": out, "bytes": n}


def run_two_graphs():
    """Two graphs through one DeviceParser: a four-tile input captured first,
    a one-tile input second (the workspace does not grow, so the first graph's
    pointer stays valid), replayed alternately twice; the large one parses A,
    then B."""
    fam, M, o, rig, split = parse_setup("libsvm_max_index")
    tile = dm.fast_geometry()[0]
    assert 3 * tile < fam["nbytes"] <= 4 * tile
    g1, _ = eager_then_capture(rig, M["A"], o["A"], split["A"])
    ws = rig.parser._ws
    lines = gc.split_lines(M["A"]["data"])
    lines = gc.fit(lines, tile // 2 + 77)
    small = {"name": "small", "data": b"".join(lines), "offs": gc.cuts_near(lines, [tile // 4]), "expect": "stay"}
    os_ = po.parse_chunks(small["data"], small["offs"], fmt=fam["fmt"], **fc.oracle_kw(rig.prm))
    assert os_["status"] == 0
    rig2 = ParseRig(fam["fmt"], None, len(small["data"]), 2, [c + gc.SLACK for c in fc.oracle_counts(os_)],
                    parser=rig.parser)
    split2 = fc.split_table(dm, small["data"], small["offs"], rig.prm)
    g2, _ = eager_then_capture(rig2, small, os_, split2)
    assert rig.parser._ws is ws and ws.data_ptr() == rig.parser._ws.data_ptr()  # one workspace serves both graphs
    order, paths = [], []
    for m in ("A", "B"):
        for r, g, mem, oo, sp in ((rig, g1, M[m], o[m], split[m]), (rig2, g2, small, os_, split2)):
            r.load(mem)
            r.refill()
            g.replay()
            h = r.collect()
            try:
                check_parse(r, h, mem, oo, sp)
            except AssertionError as e:
                raise AssertionError("%s after %s: %s" % (mem["name"], order, e))
            order.append(mem["name"])
            paths.append(h["path"])
    return {"order": order, "paths": paths}


# ---------------------------------------------------------------- chain --
def _filled(n, dtype):
    t = torch.empty(int(n), dtype=dtype, device="cuda")
    t.view(U8).fill_(gc.SENT)
    return t


def _words(t):
    a = t.cpu().numpy().reshape(-1)
    return a.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def run_chain():
    """parse_into -> gather_rows -> make_cuts(max_rows = a sample) -> to_bins,
    then to_dense and to_csc of the gathered CSR: six calls in one graph into
    upper-bound buffers, replayed in graph_cases.CHAIN_ORDER."""
    fam = gc.chain_family(geometry())
    M = fam["members"]
    o = {m: gc.chain_oracle(fam, m) for m in M}
    d = gc.chain_dims(fam, o)
    ncol, n_ids, gr, ge, G = d["ncol"], d["n_ids"], d["g_rows"], d["g_ent"], gc.GUARD
    rig = ParseRig(po.CSV, fam["kw"], fam["nbytes"], fam["nchunks"],
                   [d["rows"], d["nnz"], d["nnz"], d["rows"], d["rows"], d["rows"], d["nnz"]])
    p = rig.parser
    i64, i32, f32 = torch.int64, torch.int32, torch.float32
    shapes = {"g_offset": (gr + 1 + G, i64), "g_label": (gr + G, f32), "g_weight": (gr + G, f32), "g_qid": (gr + G, i64),
              "g_field": (ge + G, i32), "g_index": (ge + G, i32), "g_value": (ge + G, f32),
              "g_res": (16, i64), "g_status": (4, i64),
              "cut_ptr": (ncol + 1 + G, i32), "cut_value": (d["cut_cap"] + G, f32), "cuts_status": (8, i64),
              "bins": ((n_ids + G) * ncol, U8), "bins_status": (8, i64),
              "dense": ((n_ids + G) * ncol, f32), "dense_status": (4, i64),
              "csc_col_offset": (ncol + 1 + G, i64), "csc_row": (ge + G, i32), "csc_value": (ge + G, f32),
              "csc_pos": (ge + G, i64), "csc_status": (4, i64)}
    T = {k: _filled(n, dt) for k, (n, dt) in shapes.items()}
    dcsr = dm.Csr()
    for k in fc.ARRAYS:
        setattr(dcsr, k, T["g_" + k].data_ptr())
    for slot, c in ((fc.ROWS, gr), (fc.INDEX, ge), (fc.VALUE, ge), (fc.WEIGHT, gr), (fc.QID, gr), (fc.LABEL, gr),
                    (fc.FIELD, ge)):
        dcsr.cap[slot] = c
    dst = {"_csr": dcsr}
    ids = torch.empty(n_ids, dtype=i64, device="cuda")
    cut_value = T["cut_value"][:d["cut_cap"]]
    bins, dense = T["bins"].view(n_ids + G, ncol), T["dense"].view(n_ids + G, ncol)
    csc = {"col_offset": T["csc_col_offset"], "row": T["csc_row"][:ge], "value": T["csc_value"][:ge],
           "pos": T["csc_pos"][:ge]}

    def calls():
        rig.call()
        p.gather_rows_async(rig.arg, rig.res, ids, dst=dst, dst_result=T["g_res"], status=T["g_status"])
        p.make_cuts_async(dst, T["g_res"], T["cut_ptr"], cut_value, T["cuts_status"], ncol=ncol, max_bin=gc.CHAIN_MAX_BIN,
                          max_rows=gc.CHAIN_SAMPLE)
        p.to_bins_async(dst, T["g_res"], bins, T["cut_ptr"], cut_value, ncol=ncol, status=T["bins_status"])
        p.to_dense_async(dst, T["g_res"], dense, ncol=ncol, status=T["dense_status"])
        p.to_csc_async(dst, T["g_res"], csc, T["csc_status"], ncol=ncol)

    def refill():
        rig.refill()
        for t in T.values():
            t.view(U8).fill_(gc.SENT)

    def one(m, which):
        rig.load(M[m])
        ids.copy_(torch.from_numpy(fam["ids"][which]))
        refill()

    def compare(m, which):
        h = rig.collect()
        err = 0
        if M[m]["expect"] == "error":
            code, pos = M[m]["err"]
            err = (pos << 16) | code
            assert h["error"] == err, (dm.error_pos(h["error"]), dm.error_code(h["error"]), pos, code)
        else:
            assert h["error"] == 0 and h["counts"][:7] == fc.oracle_counts(o[m]), (h["error"], h["counts"])
            assert diff(h, o[m]) == [], diff(h, o[m])
            assert h["max_index"] == int(np.asarray(o[m]["index"]).max()) and h["max_field"] == 0, (h["max_index"], h["max_field"])
        want = gc.chain_expect(o[m], err, fam["ids"][which], d)
        got = {k: _words(t) for k, t in T.items()}
        got["g_res"] = got["g_res"][:12]
        bad = [k for k in want if got[k].tobytes() != np.ascontiguousarray(want[k]).tobytes()]
        assert bad == [], ("outputs that differ from the models", bad,
                           {k: (got[k][:12].tolist(), np.asarray(want[k]).reshape(-1)[:12].tolist()) for k in bad
                            if k.endswith(("status", "res"))})
        if err:  # each later call reports its error flag
            for k in ("g_status", "cuts_status", "bins_status", "dense_status", "csc_status"):
                assert int(got[k][3]) & 1, k
        return {k: v.tobytes() for k, v in got.items()}, h

    one("A", 1)
    calls()
    compare("A", 1)
    ws = (p._ws, p._gws, p._cws, p._qws)
    assert all(w is not None for w in ws)
    g = capture(calls)
    assert all(a is b for a, b in zip(ws, (p._ws, p._gws, p._cws, p._qws)))  # no workspace was allocated under the capture
    for w in ws:
        w.fill_(WS_POISON)
    seen = []
    for i, (m, which) in enumerate(gc.CHAIN_ORDER):
        one(m, which)
        g.replay()
        try:
            raw, h = compare(m, which)
        except AssertionError as e:
            raise AssertionError("replay %d (%s, ids%d): %s" % (i, m, which, e))
        seen.append((raw, h["raw"]))
    same_raw(seen[-1][0], seen[0][0], "last replay vs first")
    same_raw(seen[-1][1], seen[0][1], "last replay vs first (parse)")
    return {"order": ["%s/ids%d" % x for x in gc.CHAIN_ORDER], "n_ids": n_ids, "nbytes": fam["nbytes"], "dims": d}


def main():
    what = sys.argv[1]
    out = {"what": what, "ok": False}
    try:
        assert torch.cuda.is_available(), "GPU tests need a HIP device"
        if what.startswith("parse:"):
            out.update(run_parse(what.split(":", 1)[1]))
        else:
            out.update({"back_to_back": run_back_to_back, "copy_out": run_copy_out, "copy": run_copy,
                        "chain": run_chain, "two_graphs": run_two_graphs}[what]())
        out["ok"] = True
    except Exception as e:  # a refused capture (RuntimeError) or a replay that differs: reported, never hidden
        out["msg"] = "%s: %s" % (type(e).__name__, str(e)[:3000])
        out["trace"] = traceback.format_exc()[-1500:]
    print(json.dumps(out))
    sys.stdout.flush()
    if any(x in out.get("msg", "") for x in ("illegal memory access", "launch failure", "hardware exception")):
        os._exit(134)  # a GPU fault: the parent ends the session (nothing more may start on the GPU)


if __name__ == "__main__":
    main()
