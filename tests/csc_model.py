"""The semantics of dmlc_amd_to_csc (include/dmlc_amd.h) in numpy: what every
CSC test compares with.

    rows = min(count[ROWS], cap[ROWS]); r1 = min(rows, row_begin + max_rows)
    kept = dropped = 0; first = ~0
    for r in row_begin .. r1-1:
        for k in offset[r] .. offset[r+1]-1, ascending:      (offsets clamped to the capacity: flag 4)
            c = index[k]
            if c >= ncol: dropped += 1; first = min(first, k)
            else: append (row = r - row_begin, value[k], pos = k) to column c
    col_offset[c] = entries of columns < c, for c in 0 .. ncol

The walk visits the entries in ascending k, and a stable sort of them by column
keeps that order inside each column: numpy's argsort(kind="stable") is the
whole transpose.  Values are bit patterns (uint32 / uint64 views).
"""
import numpy as np

FLAG_ERROR, FLAG_VALUE_COUNT, FLAG_OFFSET_CAP, FLAG_CAPACITY, FLAG_MAX_ENTRIES = 1, 2, 4, 8, 16
NONE = (1 << 64) - 1


def bits(a):
    """View a float32 / int32 / int64 (or already unsigned) array as unsigned words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def passes(ncol):
    """8-bit digit passes of the device sort for ncol columns."""
    return max(1, (int(ncol - 1).bit_length() + 7) // 8)


def to_csc(offset, index, value, bufs, *, counts, ncol, error=0, cap_rows=None, cap_index=None, cap_value=None,
           row_begin=0, max_rows=None, max_entries=None):
    """-> (buffers after the call, status[4]).

    bufs: {"col_offset": uint64, "row": uint32, "value": uint32 / uint64 or
    None, "pos": uint64 or None} as the caller pre-filled them, guard words
    included; "cap" is the capacity in entries (default len(row)).
    counts: (rows, index entries, values) of the source's result block.
    value=None is a source without a value array (capacity 0)."""
    n_rows, n_index, n_value = (int(x) for x in counts)
    out = {k: (None if v is None or k == "cap" else np.array(v, copy=True)) for k, v in bufs.items()}
    cap = int(bufs.get("cap", len(bufs["row"])))
    ncol = int(ncol)
    status = [0, 0, NONE, 0]
    if error:
        status[3] |= FLAG_ERROR
    if n_value != 0 and n_value != n_index:
        status[3] |= FLAG_VALUE_COUNT
    if status[3]:
        out["col_offset"][:ncol + 1] = 0
        return out, status
    offset = np.asarray(offset, dtype=np.uint64)
    cap_rows = len(offset) - 1 if cap_rows is None else int(cap_rows)
    cap_index = len(index) if cap_index is None else int(cap_index)
    if cap_value is None:
        cap_value = 0 if value is None else len(value)
    lim = min(cap_index, cap_value) if n_value else cap_index
    rows = min(n_rows, cap_rows)
    end = rows if max_rows is None else min(rows, row_begin + int(max_rows))
    nrow = max(end - row_begin, 0)
    k = np.zeros(0, np.int64)
    row = np.zeros(0, np.int64)
    if nrow:
        off = offset[row_begin:end + 1].astype(np.int64)
        if (offset[row_begin:end + 1] > np.uint64(lim)).any():  # no element at or past the capacity is read
            status[3] |= FLAG_OFFSET_CAP
            off = np.minimum(offset[row_begin:end + 1], np.uint64(lim)).astype(np.int64)
        assert (np.diff(off) >= 0).all(), "the model is for offsets that never descend"
        k = np.arange(off[0], off[-1], dtype=np.int64)
        row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(off))
    m = cap_index if not max_entries else min(int(max_entries), cap_index)
    if len(k) > m:
        status[3] |= FLAG_MAX_ENTRIES
        k, row = k[:m], row[:m]
    col = np.asarray(index)[k].astype(np.uint64)
    keep = col < np.uint64(ncol)
    status[1] = int((~keep).sum())
    if status[1]:
        status[2] = int(k[~keep].min())
    k, row, col = k[keep], row[keep], col[keep].astype(np.int64)
    kept = len(k)
    status[0] = kept
    order = np.argsort(col, kind="stable")
    co = np.zeros(ncol + 1, np.uint64)
    co[1:] = np.cumsum(np.bincount(col, minlength=ncol)[:ncol]).astype(np.uint64)
    out["col_offset"][:ncol + 1] = co
    if kept > cap:
        status[3] |= FLAG_CAPACITY
    w = min(kept, cap)
    order = order[:w]
    out["row"][:w] = row[order].astype(np.uint32)
    if n_value and out.get("value") is not None:
        out["value"][:w] = bits(np.asarray(value))[k[order]].astype(out["value"].dtype)
    if out.get("pos") is not None:
        out["pos"][:w] = k[order].astype(np.uint64)
    return out, status
