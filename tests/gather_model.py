"""The semantics of dmlc_amd_gather_rows (include/dmlc_amd.h) in numpy: what
every gather test compares with.

    rows = min(count[ROWS], cap[ROWS])
    dst.offset[0] = 0
    for i in 0 .. n_ids-1:
        r = ids[i]
        if r >= rows: bad += 1; first_bad = min(first_bad, i); the row is empty,
                      its label / weight / qid bits are 0
        else: append index / value / field[src.offset[r] .. src.offset[r+1]) to dst,
              label / weight / qid[i] = src ...[r]
        dst.offset[i+1] = entries so far

Arrays are bit patterns (unsigned views), so NaN payloads, -0.0 and INT64_MIN
are compared exactly.  A side is a dict with the keys of ARRAYS (None = a null
pointer) and "cap", a dict slot -> capacity in elements; cap[ROWS] is also the
capacity of label, and a null array has capacity 0.
"""
import numpy as np

ROWS, INDEX, VALUE, WEIGHT, QID, LABEL, FIELD = range(7)
ARRAYS = ("offset", "label", "weight", "qid", "field", "index", "value")
FLAG_ERROR, FLAG_COUNT, FLAG_OFFSET_CAP, FLAG_CAPACITY = 1, 2, 4, 8
ERR_CAPACITY, ERR_ARG = 16, 32
NONE = (1 << 64) - 1
_SLOT = {"label": LABEL, "weight": WEIGHT, "qid": QID, "field": FIELD, "index": INDEX, "value": VALUE}


def bits(a):
    """View a float32 / int32 / int64 (or already unsigned) array as unsigned words."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def _caps(side):
    c = dict(side["cap"])
    eff = {ROWS: int(c.get(ROWS, 0)) if side.get("offset") is not None else 0}
    eff[LABEL] = eff[ROWS] if side.get("label") is not None else 0
    for name in ("weight", "qid", "field", "index", "value"):
        eff[_SLOT[name]] = int(c.get(_SLOT[name], 0)) if side.get(name) is not None else 0
    return eff


def gather_rows(src, res, ids, dst, max_index=False):
    """-> (dst arrays after the call, dst result block [16], status [4]).

    src, dst: sides as above; dst's arrays are the buffers as the caller
    pre-filled them (they are copied).  res: the source's result block (at least
    9 words: the counts and the error).  ids: unsigned ids."""
    res = [int(x) for x in res]
    res += [0] * (16 - len(res))
    ids = np.asarray(ids).astype(np.uint64)
    n = len(ids)
    out = {k: (None if dst.get(k) is None else np.array(dst[k], copy=True)) for k in ARRAYS}
    dres = [0] * 16
    status = [0, 0, NONE, 0]
    if res[8]:
        status[3] |= FLAG_ERROR
    if (res[VALUE] and res[VALUE] != res[INDEX]) or (res[FIELD] and res[FIELD] != res[INDEX]):
        status[3] |= FLAG_COUNT
    if status[3]:
        dres[8] = res[8] if res[8] else ERR_ARG
        return out, dres, status
    scap, dcap = _caps(src), _caps(dst)
    rows = min(res[ROWS], scap[ROWS])
    has = {"value": res[VALUE] != 0, "field": res[FIELD] != 0,
           "label": res[LABEL] != 0 and res[LABEL] == res[ROWS],
           "weight": res[WEIGHT] != 0 and res[WEIGHT] == res[ROWS],
           "qid": res[QID] != 0 and res[QID] == res[ROWS]}
    per_entry = ["index"] + [k for k in ("value", "field") if has[k]]
    per_row = [k for k in ("label", "weight", "qid") if has[k]]
    lim = min(scap[_SLOT[k]] for k in per_entry)
    ent_cap = min(dcap[_SLOT[k]] for k in per_entry)
    row_cap = min([dcap[ROWS]] + [dcap[_SLOT[k]] for k in per_row])

    bad = ids >= np.uint64(rows)
    status[1] = int(bad.sum())
    if status[1]:
        status[2] = int(np.flatnonzero(bad)[0])
    r = np.where(bad, 0, ids).astype(np.int64)
    if n and rows:
        off = np.asarray(src["offset"]).astype(np.uint64)
        o0, o1 = off[r], off[r + 1]
        if ((~bad) & ((o0 > lim) | (o1 > lim))).any():  # no element at or past the capacity is read
            status[3] |= FLAG_OFFSET_CAP
        o0, o1 = np.minimum(o0, np.uint64(lim)).astype(np.int64), np.minimum(o1, np.uint64(lim)).astype(np.int64)
        lens = np.where(bad | (o1 < o0), 0, o1 - o0)
    else:
        o0 = np.zeros(n, np.int64)
        lens = np.zeros(n, np.int64)
    ends = np.cumsum(lens) if n else np.zeros(0, np.int64)
    starts = ends - lens
    E = int(ends[-1]) if n else 0

    # what fits
    nw = min(n, dcap[ROWS])
    out["offset"][:nw + 1] = np.concatenate([[0], ends])[:nw + 1].astype(np.uint64)
    for k in per_row:
        m = min(n, dcap[_SLOT[k]])
        s = np.asarray(src[k]) if src.get(k) is not None else np.zeros(0, out[k].dtype)
        ok = (~bad[:m]) & (r[:m] < scap[_SLOT[k]])
        v = np.zeros(m, dtype=out[k].dtype)
        v[ok] = s[r[:m][ok]]
        out[k][:m] = v
    if E:
        pos = np.repeat(o0 - starts, lens) + np.arange(E, dtype=np.int64)  # source position of each dst entry
        for k in per_entry:
            m = min(E, dcap[_SLOT[k]])
            out[k][:m] = np.asarray(src[k])[pos[:m]]

    status[0] = nw
    dres[ROWS], dres[INDEX] = n, E
    dres[VALUE], dres[FIELD] = (E if has["value"] else 0), (E if has["field"] else 0)
    for k in ("label", "weight", "qid"):
        dres[_SLOT[k]] = n if has[k] else 0
    over = (np.arange(n) >= row_cap) | (ends > ent_cap)
    if over.any():
        status[3] |= FLAG_CAPACITY
        dres[8] = (int(np.flatnonzero(over)[0]) << 16) | ERR_CAPACITY
    if max_index:
        for k, w in (("index", 10), ("field", 11)):
            m = min(dres[_SLOT[k]], dcap[_SLOT[k]])
            dres[w] = int(out[k][:m].max()) if m else 0
    return out, dres, status


def side_from(arrays, caps=None):
    """A side from unsigned arrays (name -> array or None); capacities default to the arrays' lengths."""
    s = {k: arrays.get(k) for k in ARRAYS}
    cap = {ROWS: len(s["offset"]) - 1 if s["offset"] is not None else 0}
    for k, slot in _SLOT.items():
        if k != "label":
            cap[slot] = len(s[k]) if s[k] is not None else 0
    cap.update(caps or {})
    s["cap"] = cap
    return s
