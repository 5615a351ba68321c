"""Time dmlc_amd_to_bins on device-resident parses against the torch form a
caller would otherwise write and against dmlc_amd_to_dense of the same batch,
with an equal-bytes device copy as the bandwidth context:
python tools/time_bins.py [--out profiles/bins_times.txt]

Shapes: config 3 (synth.CSV, 1M x 256, ncol = 256) and config 2's libsvm text
(1M x 128 nnz, ncol = max_index + 1, rows cut as tools/time_dense.py cuts
them, so that the float matrix stays within 4 GiB).  256 cuts per column, the
per-column quantiles of the first 64k rows' present values; uint8 codes,
missing = 255.  Per shape, after a warm-up, `--rounds` rounds of `--calls`
calls of each form in turn, every batch of calls between two device events:
  to_bins   DeviceParser.to_bins_async into a preallocated tensor
  to_dense  DeviceParser.to_dense_async of the same rows (float32, NaN fill)
  torch     to_dense, a transposed copy, torch.searchsorted(right=True), a clamp
            and a NaN select, a narrowing copy and a transpose back
  copy      dmlc_amd_copy, device to device, of the bytes to_bins must move
            (offset + index + value read, codes written)
Before timing, the kernel's codes must equal the torch form's; afterwards
to_bins must have been faster than the torch form on both shapes.  The ratios
to to_dense and to the copy are recorded, not asserted."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "dmlc-core_amd", "python")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import dmlc_amd  # noqa: E402
from tools import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bins_times.txt"))
ap.add_argument("--calls", type=int, default=10)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--cuts", type=int, default=256)
ap.add_argument("--only", default="", help="csv or libsvm: time one shape (for a profiler run)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []
MISSING = 255


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed(fn, calls):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(calls):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / calls


def quantile_cuts(p, out, res, ncol, rows):
    """(ncol x m) per-column quantiles of the first 64k rows' present values, ascending (0.0 for an empty column)"""
    m = args.cuts
    head = min(rows, 1 << 16)
    d = torch.empty((head, ncol), dtype=torch.float32, device=dev)
    p.to_dense_async(out, res, d, ncol=ncol, max_rows=head)
    s, _ = torch.sort(d, dim=0)  # NaN (no entry) sorts last
    n = (~torch.isnan(d)).sum(dim=0)  # present values per column
    k = torch.arange(m, device=dev)[:, None] * n[None, :] // m  # (m, ncol) positions in the sorted column
    cuts = torch.gather(s, 0, k.clamp_(max=head - 1))
    cuts = torch.where(n[None, :] > 0, cuts, torch.zeros_like(cuts))
    return cuts.t().contiguous()


def shape(name, fmt, kind, width):
    text, _ = synth.rows(kind, args.rows, width, seed=1)
    starts = dmlc_amd.text_chunk_starts(text)
    p = dmlc_amd.DeviceParser(fmt, flags=dmlc_amd.FLAG_MAX_INDEX)
    out = p.parse(torch.from_numpy(text).to(dev), torch.from_numpy(starts).to(dev))
    del text
    torch.cuda.empty_cache()
    assert out["error"] == 0
    rows_all, nnz_all = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    ncol = out["max_index"] + 1
    rows = min(rows_all, (4 << 30) // (4 * ncol))
    offset, res = out["offset"], out["result"]
    nnz = int(offset[rows].item())
    m = args.cuts
    say("%s: %d x %d of the parsed %d rows (%d of %d entries), %d cuts a column, codes %.3f GiB (floats %.3f GiB), path %d"
        % (name, rows, ncol, rows_all, nnz, nnz_all, m, rows * ncol / 2**30, rows * ncol * 4 / 2**30, out["path"]))
    cuts2d = quantile_cuts(p, out, res, ncol, rows)
    cut_value = cuts2d.reshape(-1)
    cut_ptr = (torch.arange(ncol + 1, device=dev) * m).to(torch.int32)
    bins = torch.empty((rows, ncol), dtype=torch.uint8, device=dev)
    dense = torch.empty((rows, ncol), dtype=torch.float32, device=dev)
    status = torch.empty(8, dtype=torch.int64, device=dev)
    dstatus = torch.empty(4, dtype=torch.int64, device=dev)
    nbytes = (rows + 1) * 8 + nnz * 8 + rows * ncol
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f_bins():
        p.to_bins_async(out, res, bins, cut_ptr, cut_value, ncol=ncol, max_rows=rows, missing=MISSING, status=status)

    def f_dense():
        p.to_dense_async(out, res, dense, ncol=ncol, max_rows=rows, status=dstatus)

    def f_torch():
        f_dense()                                                           # 1
        dt = dense.t().contiguous()                                         # 2
        code = torch.searchsorted(cuts2d, dt, right=True, out_int32=True)   # 3
        code = torch.where(torch.isnan(dt), MISSING, code.clamp_(max=m - 1))  # 4
        return code.to(torch.uint8).t().contiguous()                        # 5

    def f_copy():
        assert dmlc_amd.lib().dmlc_amd_copy(dst.data_ptr(), src.data_ptr(), nbytes, stream) == 0

    forms = [("to_bins", f_bins), ("to_dense", f_dense), ("torch", f_torch), ("copy", f_copy)]
    # results first: the kernel's codes against the torch form's
    f_bins()
    ref = f_torch()
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint64)
    same = bool(torch.equal(bins, ref))
    say("  status rows %d dropped %d flags %d nan %d unbinned %d; equal to the torch form byte for byte: %s"
        % (st[0], st[1], st[3], st[4], st[5], same))
    assert same, "to_bins and the torch form disagree"
    del ref
    for _, fn in forms:  # warm-up
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {n: [] for n, _ in forms}
    for _ in range(args.rounds):
        for n, fn in forms:
            ms[n].append(timed(fn, args.calls))
    for n, _ in forms:
        say("  %-8s ms per call, %d calls a round: %s" % (n, args.calls, "  ".join("%.4f" % x for x in ms[n])))
    best = {n: min(v) for n, v in ms.items()}
    say("  bytes to_bins must move %.3f GB: to_bins %.0f GB/s, copy %.0f GB/s (read + write %.0f); to_bins takes %.2f x "
        "the copy's time and %.2f x to_dense's" % (nbytes / 1e9, nbytes / best["to_bins"] / 1e6, nbytes / best["copy"] / 1e6,
                                                  2 * nbytes / best["copy"] / 1e6, best["to_bins"] / best["copy"],
                                                  best["to_bins"] / best["to_dense"]))
    say("  torch / to_bins = %.2f x (rounds: %s)" % (best["torch"] / best["to_bins"],
                                                    "  ".join("%.2f" % (a / b) for a, b in zip(ms["torch"], ms["to_bins"]))))
    return max(ms["to_bins"]) < min(ms["torch"])


say("dmlc_amd_to_bins against the torch form and to_dense, MI355X, build %s, tile %d cells x %d rows"
    % ((dmlc_amd.build_id(),) + dmlc_amd.bins_geometry()))
say("(with %d cuts a column in one byte the top code equals missing = %d: every tile raises CODE_RANGE, flags 16 -- one "
    "same-address atomic a tile is part of what is timed -- and the comparison cannot tell the top bin from missing)"
    % (args.cuts, MISSING))
ok = True
if args.only in ("", "csv"):
    ok &= shape("config 3 (CSV 1M x 256)", "csv", synth.CSV, 256)
if args.only in ("", "libsvm"):
    ok &= shape("config 2 (libsvm 1M x 128 nnz)", "libsvm", synth.LIBSVM, 128)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
assert ok, "to_bins was not faster than the torch form"
