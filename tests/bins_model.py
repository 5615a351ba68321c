"""The semantics of dmlc_amd_to_bins (include/dmlc_amd.h) in numpy: what every
bins test compares with.

The window, the dropped entries and each cell's winning entry are
dmlc_amd_to_dense's, so they come from tests/dense_model.py itself: the dense
model runs over the entries' positions instead of their values, which gives
every cell the position of its winning entry (0 = no entry).  Then, for a
winning value v in column c with b = cut_ptr[c], e = cut_ptr[c + 1], m = e - b:

    b > e or e > n_cuts:  missing, unbinned += 1, flag CUT_PTR
    m == 0:               missing, unbinned += 1
    v is NaN:             missing, nan += 1
    otherwise:            x = min(searchsorted(cut_value[b:e], v, side="right"), m - 1)
                          (+ b with global_ids); a code that does not fit the
                          element or equals missing: missing, flag CODE_RANGE
"""
import numpy as np

import dense_model as dmod

FLAG_ERROR, FLAG_VALUE_COUNT, FLAG_OFFSET_CAP = dmod.FLAG_ERROR, dmod.FLAG_VALUE_COUNT, dmod.FLAG_OFFSET_CAP
FLAG_CODE_RANGE, FLAG_CUT_PTR = 16, 32
NONE = dmod.NONE
ROWS, DROPPED, FIRST, FLAGS, NAN, UNBINNED = range(6)


def search_bin(cuts, v):
    """XGBoost's HistogramCuts::SearchBin over one column's cuts (m >= 1, no NaN in v)."""
    return np.minimum(np.searchsorted(cuts, v, side="right"), len(cuts) - 1)


def codes_of(win, present, cut_ptr, cut_value, *, n_cuts=None, code_bytes=1, missing=None, global_ids=False):
    """The codes of a matrix of winning values (present: which cells have an
    entry) -> (codes as uint64, nan, unbinned, flags)."""
    cut_ptr = np.asarray(cut_ptr).astype(np.int64)
    cut_value = np.asarray(cut_value, dtype=np.float32)
    n_cuts = len(cut_value) if n_cuts is None else int(n_cuts)
    top = (1 << (8 * code_bytes)) - 1
    missing = top if missing is None else int(missing)
    codes = np.full(win.shape, missing, dtype=np.uint64)
    n_nan = n_unb = flags = 0
    for c in np.flatnonzero(present.any(axis=0)):
        rows = np.flatnonzero(present[:, c])
        b, e = int(cut_ptr[c]), int(cut_ptr[c + 1])
        if b > e or e > n_cuts:
            n_unb += len(rows)
            flags |= FLAG_CUT_PTR
            continue
        if e == b:
            n_unb += len(rows)
            continue
        v = win[rows, c].astype(np.float32)
        nan = np.isnan(v)
        n_nan += int(nan.sum())
        rows, v = rows[~nan], v[~nan]
        x = search_bin(cut_value[b:e], v).astype(np.int64) + (b if global_ids else 0)
        bad = (x > top) | (x == missing)
        if bad.any():
            flags |= FLAG_CODE_RANGE
        codes[rows[~bad], c] = x[~bad].astype(np.uint64)
    return codes, n_nan, n_unb, flags


def to_bins(offset, index, value, buf, cut_ptr, cut_value, *, counts, ncol, n_cuts=None, missing=None,
            global_ids=False, error=0, cap_rows=None, cap_index=None, row_begin=0, max_rows=None, ld=None,
            out_shift=0):
    """-> (buffer after the call, status[8]).

    buf: the whole output buffer as the caller pre-filled it (1-D uint8 /
    uint16 / uint32: its dtype is the code width); `out` starts out_shift
    elements into it.  counts: (rows, index entries, values) of the parse's
    result block.  value: float32 (bit patterns kept)."""
    n_rows, n_index, n_value = (int(x) for x in counts)
    buf = np.array(buf, copy=True)
    code_bytes = buf.dtype.itemsize
    assert buf.dtype in (np.dtype(np.uint8), np.dtype(np.uint16), np.dtype(np.uint32))
    offset = np.asarray(offset, dtype=np.uint64)
    cap = len(offset) - 1 if cap_rows is None else int(cap_rows)
    most = max(min(n_rows, cap) - int(row_begin), 0)
    if max_rows is not None:
        most = min(most, int(max_rows))
    # the dense model over positions: cell = 1 + position of the winning entry, 0 = none
    pos = np.arange(1, len(index) + 1, dtype=np.int64)
    wbuf = np.zeros(max(most, 1) * ncol, dtype=np.uint64)
    wbuf, st = dmod.to_dense(offset, index, pos, wbuf, value_dtype=np.int64,
                             counts=(n_rows, n_index, n_index if n_value == n_index or n_value == 0 else n_value),
                             ncol=ncol, fill_bits=0, error=error, cap_rows=cap_rows, cap_index=cap_index,
                             row_begin=row_begin, max_rows=max_rows)
    status = list(st) + [0, 0, 0, 0]
    if status[FLAGS] & (FLAG_ERROR | FLAG_VALUE_COUNT) or status[ROWS] == 0:
        return buf, status
    nrow = status[ROWS]
    assert nrow == most
    w = wbuf[:nrow * ncol].reshape(nrow, ncol).astype(np.int64)
    present = w > 0
    if n_value:
        vals = np.asarray(value, dtype=np.float32)
        win = np.where(present, vals[np.maximum(w - 1, 0)] if len(vals) else 0, np.float32(0)).astype(np.float32)
    else:
        win = np.ones(w.shape, dtype=np.float32)  # RowBlock::get_value: no value array means 1
    codes, status[NAN], status[UNBINNED], flags = codes_of(win, present, cut_ptr, cut_value, n_cuts=n_cuts,
                                                           code_bytes=code_bytes, missing=missing,
                                                           global_ids=global_ids)
    status[FLAGS] |= flags
    ld = ncol if ld is None else int(ld)
    assert out_shift + (nrow - 1) * ld + ncol <= len(buf)
    view = np.lib.stride_tricks.as_strided(buf[out_shift:], shape=(nrow, ncol),
                                           strides=(ld * code_bytes, code_bytes))
    view[:, :] = codes.astype(buf.dtype)
    return buf, status
