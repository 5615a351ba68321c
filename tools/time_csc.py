"""Time dmlc_amd_to_csc on device-resident parses against the torch form a
caller would otherwise write, with a device copy of one pass's bytes as the
bandwidth context:  python tools/time_csc.py [--out profiles/csc_times.txt]

Shapes: config 3 (synth.CSV, 1M x 256: ncol = 256, one digit pass), config 2's
libsvm text (1M x 128 nnz) with ncol = max_index + 1 (two passes), and config
2's arrays again under offsets that give one row half of all entries.  Per
shape, after a warm-up, `--rounds` rounds of `--calls` calls of each form in
turn, every batch of calls between two device events:
  csc     DeviceParser.to_csc_async into preallocated arrays (col_offset, row,
          value; no pos)
  torch   the indices widened to int64, torch.sort(stable=True), the row ids by
          repeat_interleave over the row lengths, index_select of the row ids
          and the values by the sort's order, col_offset by bincount + cumsum
  copy    dmlc_amd_copy, device to device, of as many bytes as one digit pass
          must move: the keys read twice (histogram, scatter), the values read,
          row and value written -- half of that sum copied, so the copy's
          read + write traffic is the pass's
Before timing, the kernel's arrays are compared with the torch form's bit for
bit.  The long-row shape must take at most twice the time of the uniform rows
of the same arrays (the tiles are cut over entries): asserted."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "csc_times.txt"))
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


def measure(name, p, out, ncol):
    """one source batch `out` (parse()'s dict); -> best ms of the csc form"""
    rows, nnz = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    offset, index, value, res = out["offset"], out["index"], out["value"], out["result"]
    longest = int((offset[1:rows + 1] - offset[:rows]).max().item())
    passes = max(1, ((ncol - 1).bit_length() + 7) // 8)
    say("%s: %d rows, %d entries, longest row %d, ncol %d (%d digit pass%s)"
        % (name, rows, nnz, longest, ncol, passes, "" if passes == 1 else "es"))
    csc = {"col_offset": torch.empty(ncol + 1, dtype=torch.int64, device=dev),
           "row": torch.empty(nnz, dtype=torch.int32, device=dev), "value": torch.empty_like(value[:nnz])}
    status = torch.empty(4, dtype=torch.int64, device=dev)
    nbytes = nnz * (4 + 4 + 4 + 4 + 4) // 2
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cdst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f_csc():
        p.to_csc_async(out, res, csc, status, ncol=ncol)

    def f_torch():
        off = offset[:rows + 1]
        keys, order = torch.sort(index[:nnz].long(), stable=True)
        rowid = torch.repeat_interleave(torch.arange(rows, device=dev, dtype=torch.int32), off[1:] - off[:-1],
                                        output_size=nnz)
        co = torch.zeros(ncol + 1, dtype=torch.int64, device=dev)
        co[1:] = torch.cumsum(torch.bincount(keys, minlength=ncol), 0)
        return {"col_offset": co, "row": rowid.index_select(0, order), "value": value[:nnz].index_select(0, order)}

    def f_copy():
        assert dmlc_amd.lib().dmlc_amd_copy(cdst.data_ptr(), src.data_ptr(), nbytes, stream) == 0

    forms = [("csc", f_csc), ("torch", f_torch), ("copy", f_copy)]
    f_csc()
    ref = f_torch()
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint64)
    same = all(bool(torch.equal(csc[k].view(torch.uint8), ref[k].view(torch.uint8))) for k in ref)
    say("  status kept %d dropped %d flags %d; equal to the torch form bit for bit: %s" % (st[0], st[1], st[3], same))
    assert same and st[0] == nnz and st[3] == 0
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
        say("  %-6s ms per call, %d calls a round: %s" % (n, args.calls, "  ".join("%.4f" % x for x in ms[n])))
    best = {n: min(v) for n, v in ms.items()}
    say("  one pass moves %.3f GB (read + write); the copy of as much takes %.4f ms (%.0f GB/s read + write): csc takes "
        "%.2f copies for %d pass%s" % (2 * nbytes / 1e9, best["copy"], 2 * nbytes / best["copy"] / 1e6,
                                        best["csc"] / best["copy"], passes, "" if passes == 1 else "es"))
    say("  torch / csc = %.2f x (rounds: %s)" % (best["torch"] / best["csc"],
                                               "  ".join("%.2f" % (a / b) for a, b in zip(ms["torch"], ms["csc"]))))
    return best["csc"]


def shape(name, fmt, kind, width, long_row=False):
    text, _ = synth.rows(kind, args.rows, width, seed=1)
    starts = dmlc_amd.text_chunk_starts(text)
    p = dmlc_amd.DeviceParser(fmt, flags=dmlc_amd.FLAG_MAX_INDEX)
    out = p.parse(torch.from_numpy(text).to(dev), torch.from_numpy(starts).to(dev))
    del text
    torch.cuda.empty_cache()
    assert out["error"] == 0
    rows, nnz = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    ncol = int(out["max_index"]) + 1
    uniform = measure(name, p, out, ncol)
    if long_row:
        # the same arrays under other offsets: row 0 holds half of all entries, the others share the rest
        half = nnz // 2
        off = torch.empty(rows + 1, dtype=torch.int64, device=dev)
        off[0] = 0
        off[1:] = half + (torch.arange(rows, device=dev, dtype=torch.int64) * (nnz - half)) // (rows - 1)
        skew = dict(out)
        skew["offset"] = off
        skewed = measure(name + ", one row holding half of all entries", p, skew, ncol)
        say("  long row / uniform rows = %.2f (must be at most 2)" % (skewed / uniform))
        assert skewed <= 2 * uniform, (skewed, uniform)


say("dmlc_amd_to_csc against the torch form, MI355X, build %s, %d entries per tile, %d bits per pass"
    % ((dmlc_amd.build_id(),) + dmlc_amd.csc_geometry()))
try:
    if args.only in ("", "csv"):
        shape("config 3 (CSV 1M x 256)", "csv", synth.CSV, 256)
    if args.only in ("", "libsvm"):
        shape("config 2 (libsvm 1M x 128 nnz)", "libsvm", synth.LIBSVM, 128, long_row=True)
finally:  # (what was measured before a failed assertion is kept)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
