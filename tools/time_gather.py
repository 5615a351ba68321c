"""Time dmlc_amd_gather_rows on device-resident parses against the torch form a
caller would otherwise write, with an equal-bytes device copy as the bandwidth
context:  python tools/time_gather.py [--out profiles/gather_times.txt]

Shapes: config 3 (synth.CSV, 1M x 256), config 2's libsvm text (1M x 128 nnz),
and config 2's arrays again under offsets that give one row half of all entries
(the documented long-row limit: one workgroup copies that row).  The ids are a
random permutation of all rows.  Per shape, after a warm-up, `--rounds` rounds
of `--calls` calls of each form in turn, every batch of calls between two
device events:
  gather  DeviceParser.gather_rows_async into preallocated arrays
  torch   row lengths from the offsets, cumsum, repeat_interleave + arange for
          the source position of every output entry, index_select per array.
          The binding keeps u32 indices and u64 offsets in int32 / int64
          tensors, so this form needs no widening copy; the positions are int64
          by construction.
  copy    dmlc_amd_copy, device to device, of the bytes the gather must move
          (ids, two offsets a row, the entries and labels read; offsets,
          entries and labels written)
Before timing, the kernel's arrays are compared with the torch form's bit for
bit."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gather_times.txt"))
ap.add_argument("--calls", type=int, default=20)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--only", default="", help="csv or libsvm: time one text (for a profiler run)")
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


def measure(name, p, out, perm):
    """one source batch `out` (parse()'s dict) and a permutation of its rows"""
    rows, nnz = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    offset, index, value, label, res = out["offset"], out["index"], out["value"], out["label"], out["result"]
    has_label = out["counts"][dmlc_amd.LABEL] == rows
    longest = int((offset[1:rows + 1] - offset[:rows]).max().item())
    say("%s: %d rows, %d entries, longest row %d, labels %s" % (name, rows, nnz, longest, has_label))
    dst = p.alloc(out["counts"])
    dres = torch.empty(16, dtype=torch.int64, device=dev)
    status = torch.empty(4, dtype=torch.int64, device=dev)
    nbytes = rows * (8 + 16) + nnz * 8 + (rows + 1) * 8 + nnz * 8 + (rows * 8 if has_label else 0)
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cdst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f_gather():
        p.gather_rows_async(out, res, perm, dst=dst, dst_result=dres, status=status)

    def f_torch():
        off = offset[:rows + 1]
        lens = (off[1:] - off[:-1])[perm]
        new_off = torch.zeros(rows + 1, dtype=torch.int64, device=dev)
        new_off[1:] = torch.cumsum(lens, 0)
        pos = torch.repeat_interleave(off[:-1][perm] - new_off[:-1], lens, output_size=nnz)
        pos += torch.arange(nnz, device=dev)
        r = {"offset": new_off, "index": index[:nnz].index_select(0, pos), "value": value[:nnz].index_select(0, pos)}
        if has_label:
            r["label"] = label[:rows].index_select(0, perm)
        return r

    def f_copy():
        assert dmlc_amd.lib().dmlc_amd_copy(cdst.data_ptr(), src.data_ptr(), nbytes, stream) == 0

    forms = [("gather", f_gather), ("torch", f_torch), ("copy", f_copy)]
    f_gather()
    ref = f_torch()
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint64)
    r = dres.cpu().numpy().view(np.uint64)
    same = all(bool(torch.equal(dst[k][:ref[k].numel()].view(torch.uint8), ref[k].view(torch.uint8))) for k in ref)
    say("  status rows %d bad %d flags %d, counts %s, error %d; equal to the torch form bit for bit: %s"
        % (st[0], st[1], st[3], [int(x) for x in r[:7]], r[8], same))
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
        say("  %-7s ms per call, %d calls a round: %s" % (n, args.calls, "  ".join("%.4f" % x for x in ms[n])))
    best = {n: min(v) for n, v in ms.items()}
    say("  bytes the gather must move %.3f GB: gather %.0f GB/s, copy %.0f GB/s (read + write %.0f), gather runs at %.2f of the copy's rate"
        % (nbytes / 1e9, nbytes / best["gather"] / 1e6, nbytes / best["copy"] / 1e6, 2 * nbytes / best["copy"] / 1e6,
           best["copy"] / best["gather"]))
    say("  torch / gather = %.2f x (rounds: %s)" % (best["torch"] / best["gather"],
                                                  "  ".join("%.2f" % (a / b) for a, b in zip(ms["torch"], ms["gather"]))))


def shape(name, fmt, kind, width, long_row=False):
    text, _ = synth.rows(kind, args.rows, width, seed=1)
    starts = dmlc_amd.text_chunk_starts(text)
    p = dmlc_amd.DeviceParser(fmt)
    out = p.parse(torch.from_numpy(text).to(dev), torch.from_numpy(starts).to(dev))
    del text
    torch.cuda.empty_cache()
    assert out["error"] == 0
    rows, nnz = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    perm = torch.randperm(rows, device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    measure(name, p, out, perm)
    if long_row:
        # the same arrays under other offsets: row 0 holds half of all entries, the others share the rest
        half = nnz // 2
        off = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        off[0] = 0
        off[1:] = half + (torch.arange(rows, device=dev, dtype=torch.int64) * (nnz - half)) // (rows - 1)
        skew = dict(out)
        skew["offset"] = off
        measure(name + ", one row holding half of all entries", p, skew, perm)


say("dmlc_amd_gather_rows against the torch form, MI355X, build %s, %d ids per tile"
    % (dmlc_amd.build_id(), dmlc_amd.gather_geometry()))
if args.only in ("", "csv"):
    shape("config 3 (CSV 1M x 256)", "csv", synth.CSV, 256)
if args.only in ("", "libsvm"):
    shape("config 2 (libsvm 1M x 128 nnz)", "libsvm", synth.LIBSVM, 128, long_row=True)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    f.write("\n".join(lines) + "\n")
