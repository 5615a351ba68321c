"""GPU tests of the capture promise of include/dmlc_amd.h: "No host
synchronisation, allocation or device-wide barrier happens inside a call, so
calls can be captured into a hipGraph."

Every device call is captured (torch.cuda.graph, global error mode, one stream,
a linear sequence) and the graph is REPLAYED over device data that changes
between replays -- what a captured epoch loop does and no eager test does:
the host-side arguments are frozen once, and whatever a launch does not reset
on the device stays stale.  The inputs are the replay families of
tests/graph_cases.py (equal byte and chunk counts; their labels are verified
on the CPU by tests/test_graph_cases.py).  Each test starts one fresh child
process (tests/graph_child.py), one after another, so that a failed capture
leaves no broken stream state for later tests; the child compares every replay
bit for bit with the oracle or the numpy models and prints one JSON line.
Nothing has a tolerance.

Pinned per parse configuration: the replay order A, B, C, A, D, A, E, A
(clean, clean with other counts and cuts, a violating line in the middle tile,
a parse error, a capacity overflow), with path == 0 for A and B and nonzero
for C; the four A replays byte-identical to one eager parse_into of A.
"""
import json
import os
import subprocess
import sys

import pytest

import graph_cases as gc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(what):
    """Run tests/graph_child.py <what>; a child that is killed by a signal,
    aborts or runs out of time ends the whole session: nothing more may start
    on a GPU after that."""
    try:
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "graph_child.py"), what], capture_output=True,
                           timeout=240)
    except subprocess.TimeoutExpired:
        pytest.exit("tests/graph_child.py %s hung on the GPU: nothing more is started there" % what, returncode=3)
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit("tests/graph_child.py %s died (%d) on the GPU: nothing more is started there\n%s"
                    % (what, r.returncode, r.stderr.decode()[-2000:]), returncode=3)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    out = json.loads(r.stdout.decode().strip().splitlines()[-1])
    assert out["ok"], "%s\n%s" % (out.get("msg"), out.get("trace"))
    return out


@pytest.mark.parametrize("config", sorted(gc.CONFIGS))
def test_gpu_graph_parse_replays(config):
    """One captured dmlc_amd_parse per configuration, replayed A, B, C, A, D,
    A, E, A: after every replay the failure status (D: error code and byte
    position; E: ERR_CAPACITY), the exact counts, every array, the unit
    table, the guard bands, max_index / max_field and the path; the A replays
    byte-identical to the eager call (all in the child)."""
    out = child("parse:" + config)
    assert out["order"] == list(gc.ORDER) and len(out["paths"]) == len(gc.ORDER) <= 8
    print("graph %s: order %s paths %s errors %s" % (config, "".join(out["order"]), out["paths"], out["errors"]))
    exact = bool(gc.CONFIGS[config][1].get("flags", 0) & gc.FLAG_EXACT)
    for m, path, err in zip(out["order"], out["paths"], out["errors"]):
        if m in "AB":
            assert (path != 0) == exact and err == 0, (m, path, err)
        if m == "C":
            assert path != 0 and err == 0, (m, path, err)
        if m == "D":
            assert err in (gc.ERR_NEG_INDEX, gc.ERR_CSV_DELIM), err
        if m == "E":
            assert err == gc.ERR_CAPACITY, err
    assert out["units"] >= 3 and (config != "libsvm_auto_index_nthread2" or out["units"] == 2 * out["nchunks"])


def test_gpu_graph_back_to_back_replays():
    """A's graph launched twice with no host work in between, then one
    synchronise: the outputs equal A's (the second launch starts from the
    state the first one left on the device)."""
    out = child("back_to_back")
    assert out["paths"] == [0]


def test_gpu_graph_copy_out():
    """The engine's sequence, parse_into then dmlc_amd_copy_n_dev into
    page-locked host arrays (host/hip_engine.h), in one graph, for A and then
    B: each host array holds exactly the replay's count of elements, equal to
    the oracle, with its sentinel tail intact."""
    out = child("copy_out")
    assert out["order"] == ["A", "B"] and out["paths"] == [0, 0]


def test_gpu_graph_copy():
    """dmlc_amd_copy, aligned (its kernels) and unaligned (its hipMemcpyAsync
    branch), each captured and replayed twice over changed source bytes."""
    out = child("copy")
    assert out["replays"] == {"aligned": 2, "unaligned": 2} and out["bytes"] % 16 == 15


def test_gpu_graph_chain():
    """parse_into -> gather_rows -> make_cuts -> to_bins, to_dense, to_csc in
    one graph, replayed A/ids1, B/ids1, A/ids2, D, A2/ids1, A/ids1: every
    word of every output and status block against the models over the
    oracle's CSR; after D the error goes down the chain; the last replay is
    byte-identical to the first."""
    out = child("chain")
    assert out["order"] == ["%s/ids%d" % x for x in gc.CHAIN_ORDER] and len(out["order"]) <= 8


def test_gpu_graph_two_graphs_through_one_parser():
    """A four-tile graph captured first and a one-tile graph second on one
    DeviceParser (one workspace, not reallocated), replayed alternately
    twice."""
    out = child("two_graphs")
    assert out["order"] == ["A", "small", "B", "small"] and out["paths"] == [0, 0, 0, 0]
