"""Time dmlc_amd_make_cuts on device-resident parses against the torch form a
caller would otherwise write, with a device copy of one pass's bytes as the
bandwidth context:  python tools/time_cuts.py [--out profiles/cuts_times.txt]

Shapes: config 3 (synth.CSV, 1M x 256: ncol = 256, five digit passes), config
2's libsvm text (1M x 128 nnz) with ncol = max_index + 1 (six passes), and
config 2's arrays again with every second entry moved to one column, which then
holds half of all entries.  Each with max_bin = 256 over the whole batch and
over its first 64k rows.  Per shape and window, after a warm-up, `--rounds`
rounds of `--calls` calls of each form in turn, every batch of calls between
two device events:
  cuts    DeviceParser.make_cuts_async into preallocated cut_ptr / cut_value
          (capacity ncol * max_bin)
  torch   the window's entries as 64-bit words column << 32 | key (the key of
          the float's bits by integer tensor ops, as include/dmlc_amd.h states
          it), one torch.sort of them, the columns' ranges and their first NaN
          by searchsorted, an ncol x max_bin gather at the ranks floor(i * n /
          max_bin), the dedupe as a mask against the previous rank, the last
          cut, masked_select and the inverse key; cut_ptr by cumsum.  The
          window's entry range is read on the host once, outside the timing
  copy    dmlc_amd_copy, device to device, of as many bytes as one digit pass
          after the first must move: the digit's word read (histogram), column
          and key read and written (scatter) -- half of that sum copied, so the
          copy's read + write traffic is the pass's
Before timing, cut_ptr and the cuts are compared with the torch form's bit for
bit.  The one-heavy-column shape must take at most twice the time of the
uniform shape of the same size (the tiles are cut over entries, and a column's
selection is max_bin picks whatever its length): asserted."""
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
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cuts_times.txt"))
ap.add_argument("--calls", type=int, default=5)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--rows", type=int, default=1 << 20)
ap.add_argument("--window", type=int, default=1 << 16)
ap.add_argument("--max-bin", type=int, default=256)
ap.add_argument("--only", default="", help="csv or libsvm: time one text (for a profiler run)")
args = ap.parse_args()
dev = torch.device("cuda", 0)
lines = []
B = args.max_bin


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


def torch_cuts(index, value, ncol):
    """-> (cut_ptr int32[ncol + 1], cut_value float32) of the entries given"""
    M = 0xFFFFFFFF
    b = value.view(torch.int32).long() & M
    b = torch.where(b == 0x80000000, torch.zeros_like(b), b)
    key = torch.where((b >> 31) != 0, ~b & M, b | 0x80000000)
    key = torch.where((b & 0x7FFFFFFF) > 0x7F800000, torch.full_like(b, M), key)
    col = index.long()
    word = ((col << 32) | key)[col < ncol]
    del b, key, col
    s, _ = torch.sort(word)
    c = torch.arange(ncol + 1, device=dev, dtype=torch.int64)
    start = torch.searchsorted(s, c << 32)
    n = torch.searchsorted(s, (c[:-1] << 32) | M) - start[:-1]  # before the column's first NaN key
    i = torch.arange(B, device=dev, dtype=torch.int64)
    pos = start[:-1, None] + (i[None, :] * n[:, None]) // B
    some = n > 0
    t = s[pos.clamp_(max=max(int(s.numel()) - 1, 0))] & M  # ncol x B
    keep = torch.zeros_like(t, dtype=torch.bool)
    keep[:, :-1] = (t[:, 1:] > t[:, :-1]) & some[:, None]
    keep[:, -1] = some
    top = s[(start[:-1] + n - 1).clamp_(min=0)] & M
    cand = torch.empty_like(t)
    cand[:, :-1] = t[:, 1:]
    cand[:, -1] = torch.where(top == 0xFF800000, top, top + 1)
    k = torch.masked_select(cand, keep)
    v = torch.where((k >> 31) != 0, k & 0x7FFFFFFF, ~k & M)
    v = torch.where(v == 0x80000000, torch.zeros_like(v), v)
    ptr = torch.zeros(ncol + 1, dtype=torch.int64, device=dev)
    ptr[1:] = torch.cumsum(keep.sum(1), 0)
    return ptr.int(), v.int().view(torch.float32)


def measure(name, p, out, ncol, max_rows):
    """one source batch `out` (parse()'s dict) and one row window; -> best ms of the cuts form"""
    rows, nnz = out["counts"][dmlc_amd.ROWS], out["counts"][dmlc_amd.INDEX]
    offset, index, value, res = out["offset"], out["index"], out["value"], out["result"]
    wrows = rows if max_rows is None else min(rows, max_rows)
    e1 = int(offset[wrows].item())
    passes = 4 + max(1, ((ncol - 1).bit_length() + 7) // 8)
    heavy = int(torch.bincount(index[:e1].long(), minlength=ncol).max().item())
    say("%s, rows [0, %d): %d entries, ncol %d, fullest column %d (%d digit passes)" % (name, wrows, e1, ncol, heavy, passes))
    cut_ptr = torch.empty(ncol + 1, dtype=torch.int32, device=dev)
    cut_value = torch.empty(ncol * B, dtype=torch.float32, device=dev)
    status = torch.empty(8, dtype=torch.int64, device=dev)
    nbytes = e1 * (4 + 8 + 8) // 2
    src = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    cdst = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream().cuda_stream

    def f_cuts():
        p.make_cuts_async(out, res, cut_ptr, cut_value, status, ncol=ncol, max_bin=B, max_rows=max_rows)

    def f_torch():
        return torch_cuts(index[:e1], value[:e1], ncol)

    def f_copy():
        assert dmlc_amd.lib().dmlc_amd_copy(cdst.data_ptr(), src.data_ptr(), nbytes, stream) == 0

    forms = [("cuts", f_cuts), ("torch", f_torch), ("copy", f_copy)]
    f_cuts()
    rptr, rval = f_torch()
    torch.cuda.synchronize()
    st = status.cpu().numpy().view(np.uint64)
    n = int(st[dmlc_amd.CUTS_N_CUTS])
    same = bool(torch.equal(cut_ptr, rptr)) and n == rval.numel() and \
        bool(torch.equal(cut_value[:n].view(torch.int32), rval.view(torch.int32)))
    say("  status kept %d dropped %d flags %d nan %d cuts %d empty columns %d; equal to the torch form bit for bit: %s"
        % (st[0], st[1], st[3], st[4], st[5], st[6], same))
    assert same and st[0] == e1 and st[3] == 0
    del rptr, rval
    for _, fn in forms:  # warm-up
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k, _ in forms}
    for _ in range(args.rounds):
        for k, fn in forms:
            ms[k].append(timed(fn, args.calls))
    for k, _ in forms:
        say("  %-6s ms per call, %d calls a round: %s" % (k, args.calls, "  ".join("%.4f" % x for x in ms[k])))
    best = {k: min(v) for k, v in ms.items()}
    say("  one pass moves %.3f GB (read + write); the copy of as much takes %.4f ms (%.0f GB/s read + write): cuts takes "
        "%.2f copies for %d passes, %.2f a pass" % (2 * nbytes / 1e9, best["copy"], 2 * nbytes / best["copy"] / 1e6,
                                                   best["cuts"] / best["copy"], passes, best["cuts"] / best["copy"] / passes))
    say("  torch / cuts = %.2f x (rounds: %s)" % (best["torch"] / best["cuts"],
                                                "  ".join("%.2f" % (a / b) for a, b in zip(ms["torch"], ms["cuts"]))))
    del src, cdst
    torch.cuda.empty_cache()
    return best["cuts"]


def shape(name, fmt, kind, width, heavy_column=False):
    text, _ = synth.rows(kind, args.rows, width, seed=1)
    starts = dmlc_amd.text_chunk_starts(text)
    p = dmlc_amd.DeviceParser(fmt, flags=dmlc_amd.FLAG_MAX_INDEX)
    out = p.parse(torch.from_numpy(text).to(dev), torch.from_numpy(starts).to(dev))
    del text
    torch.cuda.empty_cache()
    assert out["error"] == 0
    ncol = int(out["max_index"]) + 1
    uniform = measure(name, p, out, ncol, None)
    measure(name, p, out, ncol, args.window)
    if heavy_column:
        # the same arrays with every second entry moved to column 7, which then holds half of all entries
        skew = {k: v for k, v in out.items() if k != "_csr"}
        skew["index"] = out["index"].clone()
        skew["index"][::2] = 7
        skewed = measure(name + ", one column holding half of all entries", p, skew, ncol, None)
        say("  heavy column / uniform columns = %.2f (must be at most 2)" % (skewed / uniform))
        assert skewed <= 2 * uniform, (skewed, uniform)


say("dmlc_amd_make_cuts (max_bin %d) against the torch form, MI355X, build %s, %d entries per tile, %d bits per pass"
    % ((B, dmlc_amd.build_id()) + dmlc_amd.make_cuts_geometry()))
try:
    if args.only in ("", "csv"):
        shape("config 3 (CSV 1M x 256)", "csv", synth.CSV, 256)
    if args.only in ("", "libsvm"):
        shape("config 2 (libsvm 1M x 128 nnz)", "libsvm", synth.LIBSVM, 128, heavy_column=True)
finally:  # (what was measured before a failed assertion is kept)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
