"""The semantics of dmlc_amd_make_cuts (include/dmlc_amd.h) in numpy: what every
cuts test compares with.

The window, the clamping of the offsets and the dropped entries are
dmlc_amd_to_csc's (tests/csc_model.py restated: only the kept entries' columns
and values matter here).  All ordering is on the unsigned key of the float's
bits b -- no float compare, no float arithmetic:

    if b == 0x80000000: b = 0
    key = 0xffffffff if (b & 0x7fffffff) > 0x7f800000 else (~b if b >> 31 else b | 0x80000000)
    unkey(k) = k & 0x7fffffff if k >> 31 else ~k

    for c in 0 .. ncol-1:
        cut_ptr[c] = n_cuts
        s = the ascending keys of column c's non-NaN samples, n = len(s)
        if n == 0: empty += 1; continue
        t[i] = s[i * n // B] for i in 0 .. B-1
        emit unkey(t[i]) for i in 1 .. B-1 if t[i] > t[i-1]
        top = s[n-1]; last = top if top == 0xff800000 else top + 1
        emit unkey(last), bits 0x80000000 stored as 0
    cut_ptr[ncol] = n_cuts          (emit stores only below the capacity)
"""
import numpy as np

FLAG_ERROR, FLAG_VALUE_COUNT, FLAG_OFFSET_CAP, FLAG_CAPACITY, FLAG_MAX_ENTRIES = 1, 2, 4, 8, 16
NONE = (1 << 64) - 1
KEPT, DROPPED, FIRST, FLAGS, NAN, N_CUTS, EMPTY_COLS = range(7)
NAN_KEY, INF_KEY = 0xFFFFFFFF, 0xFF800000
U32, U64 = np.uint32, np.uint64


def key_of(bits):
    """uint32 float bits -> uint32 keys."""
    b = np.asarray(bits, dtype=U32).copy()
    b[b == U32(0x80000000)] = 0
    neg = (b >> U32(31)).astype(bool)
    k = np.where(neg, ~b, b | U32(0x80000000)).astype(U32)
    k[(b & U32(0x7FFFFFFF)) > U32(0x7F800000)] = NAN_KEY
    return k


def unkey(k):
    k = np.asarray(k, dtype=U32)
    return np.where((k >> U32(31)).astype(bool), k & U32(0x7FFFFFFF), ~k).astype(U32)


def passes(ncol):
    """8-bit digit passes of the device sort: four over the key, then the column's."""
    return 4 + max(1, (int(ncol - 1).bit_length() + 7) // 8)


def column_cuts(sample_bits, max_bin):
    """One column's cuts (uint32 float bits) and its NaN count, from its samples' float bits."""
    k = np.sort(key_of(sample_bits))
    n = int(np.searchsorted(k, NAN_KEY, side="left"))
    nan = len(k) - n
    if n == 0:
        return np.zeros(0, U32), nan
    s = k[:n]
    B = int(max_bin)
    t = s[(np.arange(B, dtype=np.uint64) * np.uint64(n) // np.uint64(B)).astype(np.int64)]
    cuts = list(unkey(t[1:][t[1:] > t[:-1]]))
    top = int(s[-1])
    last = int(unkey(np.array([top if top == INF_KEY else top + 1], U32))[0])
    cuts.append(0 if last == 0x80000000 else last)
    return np.array(cuts, dtype=U32), nan


def make_cuts(offset, index, value, bufs, *, counts, ncol, max_bin, error=0, cap_rows=None, cap_index=None,
              cap_value=None, row_begin=0, max_rows=None, max_entries=None):
    """-> (buffers after the call, status[8]).

    bufs: {"cut_ptr": uint32, "cut_value": uint32 (float bits)} as the caller
    pre-filled them, guard words included; "cap" is the capacity in cuts
    (default len(cut_value)).  counts: (rows, index entries, values) of the
    source's result block.  value: float32 or its uint32 bits; None is a
    source without a value array (every sample is 1.0f)."""
    n_rows, n_index, n_value = (int(x) for x in counts)
    out = {k: (None if v is None or k == "cap" else np.array(v, copy=True)) for k, v in bufs.items()}
    cap = int(bufs.get("cap", len(bufs["cut_value"])))
    ncol = int(ncol)
    status = [0, 0, NONE, 0, 0, 0, 0, 0]
    if error:
        status[FLAGS] |= FLAG_ERROR
    if n_value != 0 and n_value != n_index:
        status[FLAGS] |= FLAG_VALUE_COUNT
    if status[FLAGS]:
        out["cut_ptr"][:ncol + 1] = 0
        status[EMPTY_COLS] = ncol
        return out, status
    offset = np.asarray(offset, dtype=U64)
    cap_rows = len(offset) - 1 if cap_rows is None else int(cap_rows)
    cap_index = len(index) if cap_index is None else int(cap_index)
    if cap_value is None:
        cap_value = 0 if value is None else len(value)
    lim = min(cap_index, cap_value) if n_value else cap_index
    rows = min(n_rows, cap_rows)
    end = rows if max_rows is None else min(rows, row_begin + int(max_rows))
    k = np.zeros(0, np.int64)
    if end > row_begin:
        o0, o1 = int(offset[row_begin]), int(offset[end])
        if o0 > lim or o1 > lim:  # no element at or past the capacity is read
            status[FLAGS] |= FLAG_OFFSET_CAP
            o0, o1 = min(o0, lim), min(o1, lim)
        k = np.arange(o0, max(o1, o0), dtype=np.int64)
    m = cap_index if not max_entries else min(int(max_entries), cap_index)
    if len(k) > m:
        status[FLAGS] |= FLAG_MAX_ENTRIES
        k = k[:m]
    col = np.asarray(index)[k].astype(U64)
    keep = col < U64(ncol)
    status[DROPPED] = int((~keep).sum())
    if status[DROPPED]:
        status[FIRST] = int(k[~keep].min())
    k, col = k[keep], col[keep].astype(np.int64)
    status[KEPT] = len(k)
    if n_value:
        v = np.ascontiguousarray(np.asarray(value))
        bits = (v.view(U32) if v.dtype.itemsize == 4 else v.astype(np.float32).view(U32))[k]
    else:
        bits = np.full(len(k), 0x3F800000, U32)
    order = np.argsort(col, kind="stable")
    col, bits = col[order], bits[order]
    start = np.searchsorted(col, np.arange(ncol + 1))
    ptr = np.zeros(ncol + 1, U32)
    pieces = []
    n_cuts = 0
    for c in np.flatnonzero(np.diff(start)):
        cuts, nan = column_cuts(bits[start[c]:start[c + 1]], max_bin)
        status[NAN] += nan
        ptr[c + 1] = len(cuts)
        pieces.append(cuts)
    ptr = np.cumsum(ptr, dtype=np.uint64)
    n_cuts = int(ptr[ncol])
    status[N_CUTS] = n_cuts
    status[EMPTY_COLS] = int((np.diff(ptr.astype(np.int64)) == 0).sum())
    out["cut_ptr"][:ncol + 1] = ptr.astype(U32)
    if n_cuts > cap:
        status[FLAGS] |= FLAG_CAPACITY
    allc = np.concatenate(pieces) if pieces else np.zeros(0, U32)
    w = min(n_cuts, cap)
    out["cut_value"][:w] = allc[:w]
    return out, status
