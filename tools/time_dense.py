"""Time dmlc_amd_to_dense on device-resident parses against the torch form a
caller would otherwise write, with an equal-bytes device copy as the bandwidth
context:  python tools/time_dense.py [--out profiles/dense_times.txt]

Shapes: config 3 (synth.CSV, 1M x 256, ncol = 256) and config 2's libsvm text
(1M x 128 nnz, ncol = max_index + 1, rows cut so that the matrix stays within
4 GiB).  Per shape, after a warm-up, `--rounds` rounds of `--calls` calls of
each form in turn, every batch of calls between two device events:
  to_dense   DeviceParser.to_dense_async into a preallocated tensor
  index_put  torch.full + row ids from the offsets + index_put_
  csr        torch.sparse_csr_tensor(...).to_dense() (sums duplicates; when it runs)
  copy       dmlc_amd_copy, device to device, of the bytes the kernel must move
             (offset + index + value read, out written)
Before timing, the kernel's matrix is compared with the index_put_ form's bit
for bit (they agree where no row repeats an index)."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dense_times.txt"))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--only", default="", help="csv or libsvm: time one shape (for a profiler run)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []


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
    offset, index, value, res = out["offset"], out["index"], out["value"], out["result"]
    nnz = int(offset[rows].item())
    say("%s: %d x %d of the parsed %d rows (%d of %d entries), out %.3f GiB, path %d"
        % (name, rows, ncol, rows_all, nnz, nnz_all, rows * ncol * 4 / 2**30, out["path"]))
    dense = torch.empty((rows, ncol), dtype=torch.float32, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    nbytes = (rows + 1) * 8 + nnz * 8 + rows * ncol * 4
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    dst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f_dense():
        p.to_dense_async(out, res, dense, ncol=ncol, max_rows=rows, status=status)

    def f_index_put():
        d = torch.full((rows, ncol), float("nan"), dtype=torch.float32, device=dev)
        off = offset[:rows + 1]
        rid = torch.repeat_interleave(torch.arange(rows, device=dev), off[1:] - off[:-1], output_size=nnz)
        d.index_put_((rid, index[:nnz].long()), value[:nnz])
        return d

    def f_csr():
        return torch.sparse_csr_tensor(offset[:rows + 1], index[:nnz].long(), value[:nnz], size=(rows, ncol)).to_dense()

    def f_copy():
        assert dmlc_amd.lib().dmlc_amd_copy(dst.data_ptr(), src.data_ptr(), nbytes, stream) == 0

    forms = [("to_dense", f_dense), ("index_put", f_index_put)]
    try:
        f_csr()
        torch.cuda.synchronize()
        forms.append(("csr", f_csr))
    except Exception as e:  # not implemented for these dtypes on this build
        say("  sparse_csr_tensor(...).to_dense() does not run here: %s" % str(e).splitlines()[0][:100])
    forms.append(("copy", f_copy))
    # results: the kernel against index_put_ (missing = NaN on both sides)
    f_dense()
    ref = f_index_put()
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint64)
    same = bool(torch.equal(dense.view(torch.int32), ref.view(torch.int32)))
    say("  status rows %d dropped %d flags %d; equal to index_put_ bit for bit: %s" % (st[0], st[1], st[3], same))
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
        say("  %-9s ms per call, %d calls a round: %s" % (n, args.calls, "  ".join("%.4f" % x for x in ms[n])))
    best = {n: min(v) for n, v in ms.items()}
    say("  bytes the kernel must move %.3f GB: to_dense %.0f GB/s, copy %.0f GB/s (read + write %.0f), to_dense takes %.2f x the copy's time"
        % (nbytes / 1e9, nbytes / best["to_dense"] / 1e6, nbytes / best["copy"] / 1e6, 2 * nbytes / best["copy"] / 1e6,
           best["to_dense"] / best["copy"]))
    for n in ("index_put", "csr"):
        if n in best:
            say("  %s / to_dense = %.2f x (rounds: %s)" % (n, best[n] / best["to_dense"],
                                                        "  ".join("%.2f" % (a / b) for a, b in zip(ms[n], ms["to_dense"]))))


say("dmlc_amd_to_dense against the torch forms, MI355X, build %s, tile %d cells x %d rows"
    % ((dmlc_amd.build_id(),) + dmlc_amd.dense_geometry()))
if args.only in ("", "csv"):
    shape("config 3 (CSV 1M x 256)", "csv", synth.CSV, 256)
if args.only in ("", "libsvm"):
    shape("config 2 (libsvm 1M x 128 nnz)", "libsvm", synth.LIBSVM, 128)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
