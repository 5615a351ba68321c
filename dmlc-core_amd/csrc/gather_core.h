// gather_core.h -- row gather of a parsed CSR (dmlc_amd_gather_rows): the
// three tile bodies.  Rows ids[0 .. n_ids) of the source, in that order, become
// a new compact CSR; an id at or past the source's rows gives an empty row.
//   lengths  one workgroup per tile of kGatherRows ids: each thread looks its
//            row's two offsets up (clamped to the arrays' capacity, 0 for a bad
//            id), the block sums them, and one thread stores the tile's record
//            {entries, bad ids, first bad position, flags} in the workspace
//   scan     one workgroup: the exclusive scan of the records' entry counts,
//            in place; its first thread then sets d_status, the dst result
//            block and dst.offset[n_ids]
//   copy     one workgroup per id tile: the same lengths again, their
//            exclusive scan in LDS, dst.offset[i] and the per-row arrays; then
//            the threads stride over the tile's contiguous OUTPUT entry range
//            -- per entry, not per row, so one long row among empty ones is
//            spread over every thread (dense_core.h phase B).  Each finds its
//            entry's row in the LDS offsets; consecutive lanes store
//            consecutive elements and read consecutive elements of a source row.
// Bad ids are counted in the tile records, not by atomics on d_status: the
// status words would have to be zeroed by an earlier launch, and a record per
// tile keeps the count and the first position deterministic.  No workgroup
// waits for another; the three bodies are three plain launches.
// Everything moves as bit patterns (IT / VT = uint32_t or uint64_t).  Compiles
// as HIP device code (block.h) and as plain C++ with a host block
// (tests/emu/gather_check.cpp).
#pragma once
#include "common.h"

namespace dmlc_amd {

constexpr uint32_t kGatherRows = kThreads;          // ids per tile: one per thread
constexpr uint64_t kGatherMaxTiles = 0x7FFFFFFFull;  // one launch's grid
constexpr uint32_t kGatherRecWords = 4;              // workspace words per tile
constexpr uint64_t kGatherErrArg = 32;               // DMLC_AMD_ERR_ARG

// d_status words and flag bits (include/dmlc_amd.h)
enum { GS_ROWS = 0, GS_BAD = 1, GS_FIRST = 2, GS_FLAGS = 3 };
enum { kGatherFlagError = 1u, kGatherFlagCount = 2u, kGatherFlagOffsetCap = 4u, kGatherFlagCapacity = 8u };

// one side's arrays; cap[] is indexed by counter slot and is 0 for a null
// pointer (cap[C_LABEL] = the row capacity: dmlc_amd_csr.cap[ROWS] counts labels)
struct GatherCsr {
  uint64_t *offset;
  void *label;
  uint32_t *weight;
  uint64_t *qid;
  void *field, *index, *value;
  uint64_t cap[8];
};

struct GatherArgs {
  GatherCsr src, dst;
  const uint64_t *res;  // the source's device result block (dmlc_amd_result)
  uint64_t *dres;       // the destination's
  const void *ids;
  uint64_t n_ids;
  uint64_t ntiles;
  uint32_t id_wide;      // ids are u64 (else u32)
  uint32_t label_bytes;  // 4 | 8
  uint64_t *rec;         // workspace: ntiles records of kGatherRecWords words
  uint64_t *status;
};

// a tile's record, and the element of the block scans
struct GatherRec {
  uint64_t entries, bad, first, flags;
};
struct GatherRecAdd {
  DA_HD GatherRec operator()(const GatherRec &a, const GatherRec &b) const {
    GatherRec r;
    r.entries = a.entries + b.entries;
    r.bad = a.bad + b.bad;
    r.first = mn<uint64_t>(a.first, b.first);
    r.flags = a.flags | b.flags;
    return r;
  }
};
DA_HD GatherRec gather_rec_zero() {
  GatherRec z;
  z.entries = z.bad = z.flags = 0;
  z.first = kNone;
  return z;
}

// flag bits 0 and 1: the source parse failed, or its value / field count fits
// no RowBlock (GetBlock's CHECK, row_block.h:171-189); nothing is written then
DA_HD uint64_t gather_result_flags(const uint64_t *res) {
  uint64_t f = 0;
  if (res[8] != 0) f |= kGatherFlagError;
  if (res[C_VALUE] != 0 && res[C_VALUE] != res[C_INDEX]) f |= kGatherFlagCount;
  if (res[C_FIELD] != 0 && res[C_FIELD] != res[C_INDEX]) f |= kGatherFlagCount;
  return f;
}

// what of the source is there, from its result block and capacities
struct GatherPlan {
  uint64_t rows;     // min(count[ROWS], cap[ROWS])
  uint64_t lim;      // no source entry at or past it is read
  uint64_t ent_cap;  // the smallest dst capacity of the per-entry arrays that are written
  uint64_t row_cap;  // likewise for dst.cap[ROWS] and the per-row arrays
  bool has_val, has_field, has_label, has_weight, has_qid;
};
DA_HD GatherPlan gather_plan(const GatherArgs &a) {
  GatherPlan p;
  const uint64_t *res = a.res;
  p.rows = mn<uint64_t>(res[C_ROWS], a.src.cap[C_ROWS]);
  p.has_val = res[C_VALUE] != 0;
  p.has_field = res[C_FIELD] != 0;
  p.has_label = res[C_LABEL] != 0 && res[C_LABEL] == res[C_ROWS];
  p.has_weight = res[C_WEIGHT] != 0 && res[C_WEIGHT] == res[C_ROWS];
  p.has_qid = res[C_QID] != 0 && res[C_QID] == res[C_ROWS];
  p.lim = a.src.cap[C_INDEX];
  p.ent_cap = a.dst.cap[C_INDEX];
  if (p.has_val) {
    p.lim = mn<uint64_t>(p.lim, a.src.cap[C_VALUE]);
    p.ent_cap = mn<uint64_t>(p.ent_cap, a.dst.cap[C_VALUE]);
  }
  if (p.has_field) {
    p.lim = mn<uint64_t>(p.lim, a.src.cap[C_FIELD]);
    p.ent_cap = mn<uint64_t>(p.ent_cap, a.dst.cap[C_FIELD]);
  }
  p.row_cap = a.dst.cap[C_ROWS];
  if (p.has_label) p.row_cap = mn<uint64_t>(p.row_cap, a.dst.cap[C_LABEL]);
  if (p.has_weight) p.row_cap = mn<uint64_t>(p.row_cap, a.dst.cap[C_WEIGHT]);
  if (p.has_qid) p.row_cap = mn<uint64_t>(p.row_cap, a.dst.cap[C_QID]);
  return p;
}

// position i of ids: its source row (kNone for a bad id), the row's first
// source entry and its length, clamped to p.lim
struct GatherRow {
  uint64_t r, begin;
  GatherRec rec;
};
DA_HD GatherRow gather_row(const GatherArgs &a, const GatherPlan &p, uint64_t i) {
  GatherRow g;
  g.rec = gather_rec_zero();
  g.begin = 0;
  g.r = a.id_wide ? static_cast<const uint64_t *>(a.ids)[i] : (uint64_t) static_cast<const uint32_t *>(a.ids)[i];
  if (g.r >= p.rows) {
    g.r = kNone;
    g.rec.bad = 1;
    g.rec.first = i;
    return g;
  }
  uint64_t o0 = a.src.offset[g.r], o1 = a.src.offset[g.r + 1];
  if (o0 > p.lim || o1 > p.lim) {
    o0 = mn<uint64_t>(o0, p.lim);
    o1 = mn<uint64_t>(o1, p.lim);
    g.rec.flags = kGatherFlagOffsetCap;
  }
  g.begin = o0;
  g.rec.entries = o1 > o0 ? o1 - o0 : 0;  // (descending offsets: an empty row, nothing is read)
  return g;
}

// ---- lengths: the tile's record
template <class BK>
DA_HDF void gather_lengths_tile(const GatherArgs &a, uint64_t tile, BK &bk) {
  if (gather_result_flags(a.res) != 0) return;  // (uniform) the scan does not read the records then
  const GatherPlan p = gather_plan(a);
  const uint64_t i = tile * kGatherRows + (uint32_t)bk.tid();
  GatherRec mine = gather_rec_zero();
  if (i < a.n_ids) mine = gather_row(a, p, i).rec;
  GatherRec total;
  (void)bk.exclusive(mine, gather_rec_zero(), GatherRecAdd(), &total);
  if (bk.tid() == 0) {
    uint64_t *rec = a.rec + tile * kGatherRecWords;
    rec[0] = total.entries;
    rec[1] = total.bad;
    rec[2] = total.first;
    rec[3] = total.flags;
  }
}

// ---- scan: rec[k][0] becomes the entries before tile k; d_status, the dst
// result block and dst.offset[n_ids]
template <class BK>
DA_HDF void gather_scan(const GatherArgs &a, BK &bk) {
  const uint64_t sflags = gather_result_flags(a.res);
  const uint32_t tid = (uint32_t)bk.tid();
  if (sflags != 0) {  // (uniform) nothing is written: zero counts, the source's error
    if (tid == 0) {
      a.status[GS_ROWS] = 0;
      a.status[GS_BAD] = 0;
      a.status[GS_FIRST] = kNone;
      a.status[GS_FLAGS] = sflags;
      for (int k = 0; k < 16; ++k) a.dres[k] = 0;
      a.dres[8] = a.res[8] != 0 ? a.res[8] : kGatherErrArg;
    }
    return;
  }
  const uint64_t per = (a.ntiles + kThreads - 1) / kThreads;
  const uint64_t t0 = mn<uint64_t>((uint64_t)tid * per, a.ntiles), t1 = mn<uint64_t>(t0 + per, a.ntiles);
  GatherRec mine = gather_rec_zero();
  for (uint64_t k = t0; k < t1; ++k) {
    const uint64_t *rec = a.rec + k * kGatherRecWords;
    GatherRec x;
    x.entries = rec[0];
    x.bad = rec[1];
    x.first = rec[2];
    x.flags = rec[3];
    mine = GatherRecAdd()(mine, x);
  }
  GatherRec total;
  const GatherRec ex = bk.exclusive(mine, gather_rec_zero(), GatherRecAdd(), &total);
  uint64_t run = ex.entries;
  for (uint64_t k = t0; k < t1; ++k) {
    uint64_t *rec = a.rec + k * kGatherRecWords;
    const uint64_t n = rec[0];
    rec[0] = run;
    run += n;
  }
  if (tid == 0) {
    const GatherPlan p = gather_plan(a);
    const uint64_t E = total.entries;
    const bool over = a.n_ids > p.row_cap || E > p.ent_cap;
    a.status[GS_ROWS] = mn<uint64_t>(a.n_ids, a.dst.cap[C_ROWS]);
    a.status[GS_BAD] = total.bad;
    a.status[GS_FIRST] = total.first;
    a.status[GS_FLAGS] = total.flags | (over ? (uint64_t)kGatherFlagCapacity : 0);
    uint64_t *d = a.dres;
    for (int k = 0; k < 16; ++k) d[k] = 0;  // error (the copy's one overflowing thread sets it), path, maxima
    d[C_ROWS] = a.n_ids;
    d[C_INDEX] = E;
    d[C_VALUE] = p.has_val ? E : 0;
    d[C_FIELD] = p.has_field ? E : 0;
    d[C_LABEL] = p.has_label ? a.n_ids : 0;
    d[C_WEIGHT] = p.has_weight ? a.n_ids : 0;
    d[C_QID] = p.has_qid ? a.n_ids : 0;
    if (a.n_ids <= a.dst.cap[C_ROWS] && a.dst.offset) a.dst.offset[a.n_ids] = E;
  }
}

// ---- copy.  dpos: kGatherRows + 1 words (the rows' first dst entries and the
// tile's end), spos: kGatherRows words (their first source entries)
template <typename IT, typename VT, class BK>
DA_HDF void gather_copy_tile(const GatherArgs &a, uint64_t tile, uint64_t *dpos, uint64_t *spos, BK &bk) {
  if (gather_result_flags(a.res) != 0) return;
  const GatherPlan p = gather_plan(a);
  const uint32_t tid = (uint32_t)bk.tid();
  const uint64_t i0 = tile * kGatherRows;
  const uint32_t nr = (uint32_t)mn<uint64_t>(kGatherRows, a.n_ids - i0);
  const uint64_t i = i0 + tid;
  GatherRow g;
  g.r = kNone;
  g.begin = 0;
  g.rec = gather_rec_zero();
  if (tid < nr) g = gather_row(a, p, i);
  uint64_t tile_entries;
  struct Add {
    DA_HD uint64_t operator()(uint64_t x, uint64_t y) const { return x + y; }
  };
  const uint64_t e0 = a.rec[tile * kGatherRecWords];
  const uint64_t mine = e0 + bk.exclusive(g.rec.entries, (uint64_t)0, Add(), &tile_entries);
  const uint64_t e1 = e0 + tile_entries;
  dpos[tid] = mine;  // (threads past nr: the tile's end)
  spos[tid] = g.begin;
  if (tid == 0) dpos[kGatherRows] = e1;

  // the row's own words
  if (tid < nr) {
    if (i <= a.dst.cap[C_ROWS] && a.dst.offset) a.dst.offset[i] = mine;
    const bool ok = g.r != kNone;
    if (p.has_label && i < a.dst.cap[C_LABEL]) {
      const bool rd = ok && g.r < a.src.cap[C_LABEL];
      if (a.label_bytes == 8) static_cast<uint64_t *>(a.dst.label)[i] = rd ? static_cast<const uint64_t *>(a.src.label)[g.r] : 0;
      else static_cast<uint32_t *>(a.dst.label)[i] = rd ? static_cast<const uint32_t *>(a.src.label)[g.r] : 0;
    }
    if (p.has_weight && i < a.dst.cap[C_WEIGHT]) a.dst.weight[i] = ok && g.r < a.src.cap[C_WEIGHT] ? a.src.weight[g.r] : 0;
    if (p.has_qid && i < a.dst.cap[C_QID]) a.dst.qid[i] = ok && g.r < a.src.cap[C_QID] ? a.src.qid[g.r] : 0;
    // the first position whose row or entries do not fit: "does not fit" is
    // monotone in i, so exactly one thread of the launch sees the step
    const uint64_t end = mine + g.rec.entries;
    const bool over = i >= p.row_cap || end > p.ent_cap;
    const bool before = i > 0 && (i - 1 >= p.row_cap || mine > p.ent_cap);
    if (over && !before) a.dres[8] = (i << 16) | (uint64_t)E_CAPACITY;
  }
  bk.sync();

  // the entries
  if (e1 == e0) return;
  const IT *sindex = static_cast<const IT *>(a.src.index);
  const VT *svalue = static_cast<const VT *>(a.src.value);
  const IT *sfield = static_cast<const IT *>(a.src.field);
  IT *dindex = static_cast<IT *>(a.dst.index);
  VT *dvalue = static_cast<VT *>(a.dst.value);
  IT *dfield = static_cast<IT *>(a.dst.field);
  const uint64_t cap_i = a.dst.cap[C_INDEX];
  const uint64_t cap_v = p.has_val ? a.dst.cap[C_VALUE] : 0;
  const uint64_t cap_f = p.has_field ? a.dst.cap[C_FIELD] : 0;
  const uint64_t stop = mn<uint64_t>(e1, mx<uint64_t>(cap_i, mx<uint64_t>(cap_v, cap_f)));  // nothing past every capacity
  const float scale = (float)nr / (float)(e1 - e0);
  for (uint64_t k = e0 + tid; k < stop; k += kThreads) {
    // the entry's row: the last j with dpos[j] <= k (empty rows share a
    // position with their successor).  Rows of equal length are found by the
    // first guess; otherwise a binary search from it.
    uint32_t gs = (uint32_t)((float)(k - e0) * scale);
    gs = gs < nr ? gs : nr - 1;
    uint32_t lo, hi;
    if (dpos[gs] <= k) {
      lo = gs;
      hi = dpos[gs + 1] > k ? gs + 1 : nr;
    } else {
      lo = 0;
      hi = gs;
    }
    while (hi - lo > 1) {
      const uint32_t mid = (lo + hi) >> 1;
      if (dpos[mid] <= k) lo = mid;
      else hi = mid;
    }
    const uint64_t s = spos[lo] + (k - dpos[lo]);  // (< p.lim: the row's clamped range)
    if (k < cap_i) dindex[k] = sindex[s];
    if (k < cap_v) dvalue[k] = svalue[s];
    if (k < cap_f) dfield[k] = sfield[s];
  }
}

}  // namespace dmlc_amd
