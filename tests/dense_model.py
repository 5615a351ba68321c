"""The semantics of dmlc_amd_to_dense (include/dmlc_amd.h) in numpy: what
every dense test compares with.

    rows = min(count[ROWS], cap[ROWS])
    for r in row_begin .. min(rows, row_begin + max_rows) - 1:
        out[(r - row_begin) * ld + 0..ncol-1] = fill
        for k in offset[r] .. offset[r+1]-1, ascending:
            c = index[k]
            if c < ncol: out[(r - row_begin) * ld + c] = 1 if count[VALUE] == 0 else value[k]
            else:        dropped += 1; first_dropped = min(first_dropped, k)

Cells are bit patterns (uint32 / uint64 views), so -0.0, NaN payloads and
INT64_MIN are compared exactly.  NumPy's assignment through repeated indices
keeps the last value, which is the "last entry wins" of the walk above (the
entries are assigned in ascending k).
"""
import numpy as np

FLAG_ERROR, FLAG_VALUE_COUNT, FLAG_OFFSET_CAP = 1, 2, 4
NONE = (1 << 64) - 1
_ONE = {np.dtype(np.float32): 0x3F800000, np.dtype(np.int32): 1, np.dtype(np.int64): 1}


def bits(a):
    """View a float32 / int32 / int64 (or already unsigned) array as unsigned words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def to_dense(offset, index, value, buf, *, value_dtype, counts, ncol, fill_bits, error=0, cap_rows=None,
             cap_index=None, row_begin=0, max_rows=None, ld=None, out_shift=0):
    """-> (buffer after the call, status[4]).

    buf: the whole output buffer as the caller pre-filled it (1-D, unsigned
    words of the value type's size); `out` starts out_shift elements into it.
    counts: (rows, index entries, values) of the parse's result block.
    value_dtype decides the 1 of a CSR without values."""
    n_rows, n_index, n_value = (int(x) for x in counts)
    buf = np.array(buf, copy=True)
    word = buf.dtype
    assert word in (np.dtype(np.uint32), np.dtype(np.uint64))
    status = [0, 0, NONE, 0]
    if error:
        status[3] |= FLAG_ERROR
    if n_value != 0 and n_value != n_index:
        status[3] |= FLAG_VALUE_COUNT
    if status[3]:
        return buf, status
    offset = np.asarray(offset, dtype=np.uint64)
    cap_rows = len(offset) - 1 if cap_rows is None else int(cap_rows)
    cap_index = len(index) if cap_index is None else int(cap_index)
    ld = ncol if ld is None else int(ld)
    rows = min(n_rows, cap_rows)
    end = rows if max_rows is None else min(rows, row_begin + int(max_rows))
    nrow = max(end - row_begin, 0)
    status[0] = nrow
    if nrow == 0:
        return buf, status
    off = offset[row_begin:end + 1].astype(np.int64)
    if (off > cap_index).any():  # no element at or past the capacity is read
        status[3] |= FLAG_OFFSET_CAP
        off = np.minimum(off, cap_index)
    k = np.arange(off[0], off[-1], dtype=np.int64)
    row = np.repeat(np.arange(nrow, dtype=np.int64), np.diff(off))
    col = np.asarray(index)[k].astype(np.uint64)
    keep = col < np.uint64(ncol)
    status[1] = int((~keep).sum())
    if status[1]:
        status[2] = int(k[~keep].min())
    if n_value:
        val = bits(np.asarray(value))[k].astype(word)
    else:
        val = np.full(len(k), _ONE[np.dtype(value_dtype)], dtype=word)
    mask = (1 << (8 * word.itemsize)) - 1
    view = np.lib.stride_tricks.as_strided(buf[out_shift:], shape=(nrow, ncol),
                                           strides=(ld * word.itemsize, word.itemsize))
    assert out_shift + (nrow - 1) * ld + ncol <= len(buf)
    view[:, :] = word.type(int(fill_bits) & mask)
    view[row[keep], col[keep].astype(np.int64)] = val[keep]
    return buf, status
