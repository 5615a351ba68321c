// cuts_core.h -- per-column quantile cut points of a parsed CSR
// (dmlc_amd_make_cuts): the tile bodies.  The window's kept entries are sorted
// by (column, key), key being the order-preserving unsigned form of the float's
// bits, as an LSD radix sort over 8-bit digits: four passes over the key, then
// P = ceil(bits(ncol - 1) / 8) passes over the column, three plain launches a
// pass.  The sort restates csc_core.h's (hist, scan, scatter; the ballot ranks,
// the tile records for the dropped entries) instead of sharing it: csc.hip's
// kernels keep their code and their resource lines.  Tiles are kCutsTile
// consecutive ENTRIES, so one column holding half of all entries is spread over
// every tile.
//   hist     one workgroup per tile: the tile's 256 digit counts to
//            hist[digit][tile]; pass 0 reads index / value over the window,
//            builds the keys, counts only entries with index < ncol and stores
//            the tile's record {dropped, first dropped position, flags}
//   scan     256 workgroups, one per digit: the exclusive scan of the digit's
//            row of tile counts in place, and the digit's total; after pass 0
//            workgroup 0 sums the records into meta
//   scatter  one workgroup per tile: ranks the entries stably by eight ballots
//            a round, orders the tile's (column, key) by digit in LDS and
//            stores each digit's run to the other buffer with consecutive
//            lanes on consecutive words
//   bounds   cstart[c] = the first sorted entry with column >= c, c in 0 .. ncol
//   count    one workgroup per column (grid-stride): n = the column's samples
//            before its first NaN key, and the cuts it will hold, to cut_ptr[c]
//   ptr      one workgroup: the exclusive scan of cut_ptr in place, and d_status
//   write    one workgroup per column: the deduplicated rank picks and the last
//            cut, every store checked against the capacity
// A column's work in count / write is max_bin picks whatever its length, so a
// column of half the entries costs what any other costs.  No workgroup waits
// for another.  Compiles as HIP device code (block.h) and as plain C++ with a
// host block (tests/emu/cuts_check.cpp).
#pragma once
#include "common.h"

namespace dmlc_amd {

constexpr uint32_t kCutsRounds = 16;                       // entries per thread
constexpr uint32_t kCutsTile = kThreads * kCutsRounds;     // entries per tile
constexpr uint32_t kCutsWaveRun = kWave * kCutsRounds;     // consecutive entries of one wave
constexpr uint32_t kCutsRadixBits = 8;
constexpr uint32_t kCutsDigits = 1u << kCutsRadixBits;     // == kThreads: one digit per thread / scan workgroup
constexpr uint32_t kCutsKeyPasses = 32 / kCutsRadixBits;   // digit passes over the key
constexpr uint32_t kCutsRecWords = 4;                      // workspace words per tile record
constexpr uint64_t kCutsMaxWindow = 0xFFFFFFFFull;         // a window of this many rows or entries is refused
constexpr uint32_t kCutsMaxGrid = 1u << 20;                // workgroups of count / write (they stride over the columns)
constexpr uint32_t kCutsNanKey = 0xFFFFFFFFu;              // any NaN: sorts last, is no sample
constexpr uint32_t kCutsInfKey = 0xFF800000u;              // +inf: the one key whose successor is not taken
constexpr uint32_t kCutsOneKey = 0xBF800000u;              // 1.0f: every sample of a source without values
static_assert(kCutsDigits == (uint32_t)kThreads, "one digit per thread");
static_assert(kCutsWaveRun <= 0x10000u, "a wave-local rank fits 16 bits");

// d_status words and flag bits (include/dmlc_amd.h)
enum { CU_KEPT = 0, CU_DROPPED = 1, CU_FIRST = 2, CU_FLAGS = 3, CU_NAN = 4, CU_NCUTS = 5, CU_EMPTY = 6, CU_ZERO = 7 };
enum {
  kCutsFlagError = 1u,
  kCutsFlagValueCount = 2u,
  kCutsFlagOffsetCap = 4u,
  kCutsFlagCapacity = 8u,
  kCutsFlagMaxEntries = 16u
};

struct CutsArgs {
  const uint64_t *offset;
  const void *index;
  const uint32_t *value;  // float bits
  const uint64_t *res;    // the source's device result block (dmlc_amd_result)
  uint64_t cap_rows, cap_index, cap_value;
  uint64_t row_begin, row_end;  // the row window (row_end saturates)
  uint64_t ncol;
  uint64_t max_entries;  // the launches are sized for this many entries
  uint64_t ntiles;       // tiles launched, and the stride of hist's digit rows
  uint32_t max_bin;
  uint32_t passes, pass;  // kCutsKeyPasses + the column's digit passes
  // outputs
  uint32_t *cut_ptr;
  uint32_t *cut_value;  // float bits
  uint64_t cap;
  uint64_t *status;
  // workspace
  uint64_t *meta;   // kept, dropped, first, flags (set by the scan of pass 0)
  uint32_t *total;  // kCutsDigits digit totals of the current pass
  uint64_t *rec;    // ntiles records of kCutsRecWords words
  uint32_t *hist;   // kCutsDigits rows of ntiles counts
  uint32_t *col[2], *key[2];  // the carried (column, key), max_entries each
  uint32_t *cstart;           // ncol + 1: each column's first sorted entry
  uint32_t *cn;               // ncol: each column's samples
};

// the order-preserving key of a float's bits and its inverse
DA_HD uint32_t cuts_key(uint32_t b) {
  if (b == 0x80000000u) b = 0;  // -0.0 counts as +0.0
  if ((b & 0x7FFFFFFFu) > 0x7F800000u) return kCutsNanKey;
  return (b >> 31) ? ~b : (b | 0x80000000u);
}
DA_HD uint32_t cuts_unkey(uint32_t k) { return (k >> 31) ? (k & 0x7FFFFFFFu) : ~k; }

// digit passes over the column for ncol columns
DA_HD uint32_t cuts_col_passes(uint64_t ncol) {
  uint32_t p = 1;
  for (uint64_t m = (ncol - 1) >> kCutsRadixBits; m != 0; m >>= kCutsRadixBits) ++p;
  return p;
}
DA_HD uint32_t cuts_digit(uint32_t pass, uint32_t col, uint32_t key) {
  const uint32_t v = pass < kCutsKeyPasses ? key >> (pass * kCutsRadixBits) : col >> ((pass - kCutsKeyPasses) * kCutsRadixBits);
  return v & (kCutsDigits - 1);
}

// flag bits 0 and 1: the parse failed, or its value count fits no RowBlock;
// nothing is sorted then (ptr sets every cut_ptr word to 0)
DA_HD uint64_t cuts_result_flags(const uint64_t *res) {
  uint64_t f = 0;
  if (res[8] != 0) f |= kCutsFlagError;
  if (res[C_VALUE] != 0 && res[C_VALUE] != res[C_INDEX]) f |= kCutsFlagValueCount;
  return f;
}

// the window: its entries [e0, e0 + E), no source element at or past lim is read
struct CutsWin {
  uint64_t e0, E, lim, flags;
  bool has_val;
};
DA_HD CutsWin cuts_window(const CutsArgs &a) {
  CutsWin w;
  w.has_val = a.res[C_VALUE] != 0;
  w.lim = w.has_val ? mn<uint64_t>(a.cap_index, a.cap_value) : a.cap_index;
  w.flags = 0;
  w.e0 = w.E = 0;
  const uint64_t r0 = a.row_begin;
  const uint64_t r1 = mn<uint64_t>(mn<uint64_t>(a.res[C_ROWS], a.cap_rows), a.row_end);
  if (r1 <= r0) return w;  // an empty window
  uint64_t o0 = a.offset[r0], o1 = a.offset[r1];
  if (o0 > w.lim || o1 > w.lim) {
    o0 = mn<uint64_t>(o0, w.lim);
    o1 = mn<uint64_t>(o1, w.lim);
    w.flags |= kCutsFlagOffsetCap;
  }
  w.e0 = o0;
  w.E = o1 > o0 ? o1 - o0 : 0;  // (descending offsets: nothing is read)
  if (w.E > a.max_entries) {    // the launches hold no more
    w.E = a.max_entries;
    w.flags |= kCutsFlagMaxEntries;
  }
  return w;
}

// entries the current pass sorts: the window's in pass 0, the kept ones after it
DA_HD uint64_t cuts_pass_entries(const CutsArgs &a, const CutsWin &w) { return a.pass == 0 ? w.E : a.meta[CU_KEPT]; }

struct CutsRec {
  uint64_t dropped, first;
};
struct CutsRecAdd {
  DA_HD CutsRec operator()(const CutsRec &x, const CutsRec &y) const {
    CutsRec r;
    r.dropped = x.dropped + y.dropped;
    r.first = mn<uint64_t>(x.first, y.first);
    return r;
  }
};
DA_HD CutsRec cuts_rec_zero() {
  CutsRec z;
  z.dropped = 0;
  z.first = kNone;
  return z;
}
struct CutsAdd {
  DA_HD uint64_t operator()(uint64_t x, uint64_t y) const { return x + y; }
};
// what ptr sums over the columns
struct CutsSum {
  uint64_t cuts, n, empty;
};
struct CutsSumAdd {
  DA_HD CutsSum operator()(const CutsSum &x, const CutsSum &y) const {
    CutsSum r;
    r.cuts = x.cuts + y.cuts;
    r.n = x.n + y.n;
    r.empty = x.empty + y.empty;
    return r;
  }
};
DA_HD CutsSum cuts_sum_zero() {
  CutsSum z;
  z.cuts = z.n = z.empty = 0;
  return z;
}

// pass 0: entry k of the source as (kept, column, key)
template <typename IT>
DA_HD bool cuts_source(const CutsArgs &a, const CutsWin &w, uint64_t k, uint32_t *col, uint32_t *key) {
  const uint64_t c = (uint64_t) static_cast<const IT *>(a.index)[k];
  if (c >= a.ncol) return false;
  *col = (uint32_t)c;
  *key = w.has_val ? cuts_key(a.value[k]) : kCutsOneKey;  // (k < lim: the window's clamped range)
  return true;
}

// ---- hist.  cnt: kCutsDigits words
template <typename IT, class BK>
DA_HDF void cuts_hist_tile(const CutsArgs &a, uint64_t tile, uint32_t *cnt, BK &bk) {
  if (cuts_result_flags(a.res) != 0) return;  // (uniform) nothing reads the counts then
  const CutsWin w = cuts_window(a);
  const uint64_t n = cuts_pass_entries(a, w);
  const uint64_t i0 = tile * kCutsTile;
  if (i0 >= n) return;  // (uniform) past the real count: the scan reads ceil(n / tile) tiles
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t nl = (uint32_t)mn<uint64_t>(kCutsTile, n - i0);
  cnt[tid] = 0;
  bk.sync();
  CutsRec mine = cuts_rec_zero();
  if (a.pass == 0) {
    const uint64_t k0 = w.e0 + i0;
    for (uint32_t i = tid; i < nl; i += kThreads) {
      uint32_t col = 0, key = 0;
      if (!cuts_source<IT>(a, w, k0 + i, &col, &key)) {
        ++mine.dropped;
        mine.first = mn<uint64_t>(mine.first, k0 + i);
      } else {
        (void)atomic_add_u32(&cnt[cuts_digit(0, col, key)], 1u);
      }
    }
  } else {
    const uint32_t *col = a.col[(a.pass - 1) & 1] + i0, *key = a.key[(a.pass - 1) & 1] + i0;
    if (a.pass < kCutsKeyPasses) {
      for (uint32_t i = tid; i < nl; i += kThreads) (void)atomic_add_u32(&cnt[cuts_digit(a.pass, 0, key[i])], 1u);
    } else {
      for (uint32_t i = tid; i < nl; i += kThreads) (void)atomic_add_u32(&cnt[cuts_digit(a.pass, col[i], 0)], 1u);
    }
  }
  bk.sync();
  a.hist[(uint64_t)tid * a.ntiles + tile] = cnt[tid];
  if (a.pass == 0) {
    CutsRec total;
    (void)bk.exclusive(mine, cuts_rec_zero(), CutsRecAdd(), &total);
    if (tid == 0) {
      uint64_t *rec = a.rec + tile * kCutsRecWords;
      rec[0] = total.dropped;
      rec[1] = total.first;
      rec[2] = w.flags;
      rec[3] = 0;
    }
  }
}

// ---- scan: workgroup `digit` scans hist[digit][0 .. tiles) in place
template <class BK>
DA_HDF void cuts_scan(const CutsArgs &a, uint32_t digit, BK &bk) {
  if (cuts_result_flags(a.res) != 0) return;  // (uniform) ptr sets the status and cut_ptr
  const uint32_t tid = (uint32_t)bk.tid();
  const CutsWin w = cuts_window(a);
  const uint64_t n = cuts_pass_entries(a, w);
  const uint64_t nt = n / kCutsTile + (n % kCutsTile != 0);  // (<= a.ntiles: n <= max_entries)
  const uint64_t per = (nt + kThreads - 1) / kThreads;
  const uint64_t t0 = mn<uint64_t>((uint64_t)tid * per, nt), t1 = mn<uint64_t>(t0 + per, nt);
  uint32_t *h = a.hist + (uint64_t)digit * a.ntiles;
  uint64_t mine = 0;
  for (uint64_t k = t0; k < t1; ++k) mine += h[k];
  uint64_t total;
  uint64_t run = bk.exclusive(mine, (uint64_t)0, CutsAdd(), &total);
  for (uint64_t k = t0; k < t1; ++k) {
    const uint32_t c = h[k];
    h[k] = (uint32_t)run;
    run += c;
  }
  if (tid == 0) a.total[digit] = (uint32_t)total;
  if (a.pass != 0 || digit != 0) return;  // (uniform)
  // the records' sums: what every later launch sizes itself by
  CutsRec r = cuts_rec_zero();
  for (uint64_t k = t0; k < t1; ++k) {
    CutsRec x;
    x.dropped = a.rec[k * kCutsRecWords];
    x.first = a.rec[k * kCutsRecWords + 1];
    r = CutsRecAdd()(r, x);
  }
  CutsRec all;
  (void)bk.exclusive(r, cuts_rec_zero(), CutsRecAdd(), &all);
  if (tid == 0) {
    a.meta[CU_KEPT] = w.E - all.dropped;
    a.meta[CU_DROPPED] = all.dropped;
    a.meta[CU_FIRST] = all.first;
    a.meta[CU_FLAGS] = w.flags;
  }
}

// ---- scatter.  cnt: kWaves * kCutsDigits words; stage: 2 * kCutsTile words; gdelta: kCutsDigits + 1 words
// kFirst: pass 0, which reads the source (IT: its index type); the later passes read the other buffer
template <typename IT, bool kFirst, class BK>
DA_HDF void cuts_scatter_tile(const CutsArgs &a, uint64_t tile, uint32_t *cnt, uint32_t *stage, uint32_t *gdelta, BK &bk) {
  if (cuts_result_flags(a.res) != 0) return;
  const CutsWin w = cuts_window(a);
  const uint64_t n = cuts_pass_entries(a, w);
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t lane = tid & (kWave - 1), wv = tid / kWave;

  const uint64_t i0 = tile * kCutsTile;
  if (i0 >= n) return;  // (uniform) past the real count
  const uint32_t nl = (uint32_t)mn<uint64_t>(kCutsTile, n - i0);
  for (uint32_t j = 0; j < (uint32_t)kWaves; ++j) cnt[j * kCutsDigits + tid] = 0;
  const uint32_t *scol = a.col[(a.pass + 1) & 1], *skey = a.key[(a.pass + 1) & 1];  // (pass > 0: what pass - 1 wrote)
  uint32_t *dcol = a.col[a.pass & 1], *dkey = a.key[a.pass & 1];
  const uint64_t k0 = w.e0 + i0;  // pass 0: the tile's first source position
  bk.sync();

  // ranks: tag = valid | digit << 16 | rank among the wave's earlier entries of the digit
  uint32_t tag[kCutsRounds];
#pragma unroll
  for (uint32_t r = 0; r < kCutsRounds; ++r) {
    const uint32_t i = wv * kCutsWaveRun + r * kWave + lane;
    bool valid = i < nl;
    uint32_t col = 0, key = 0;
    if (valid) {
      if (kFirst) {
        valid = cuts_source<IT>(a, w, k0 + i, &col, &key);
      } else if (a.pass < kCutsKeyPasses) {
        key = skey[i0 + i];
      } else {
        col = scol[i0 + i];
      }
    }
    const uint32_t d = cuts_digit(a.pass, col, key);
    uint64_t peers = bk.ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < kCutsRadixBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = bk.ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t below = (uint32_t)popc64(peers & ((1ull << lane) - 1));
    uint32_t *slot = &cnt[wv * kCutsDigits + d];
    const uint32_t prev = valid ? *slot : 0;
    bk.wave_sync();
    if (valid && below == 0) *slot = prev + (uint32_t)popc64(peers);
    bk.wave_sync();
    tag[r] = valid ? (0x80000000u | (d << 16) | (prev + below)) : 0u;
  }
  bk.sync();

  // the tile's entries in digit order: a thread per digit scans the waves'
  // counts, the digits' counts are scanned over the block, and every entry gets
  // a place in the LDS stage; gdelta[d] = the digit's first destination minus
  // its first place (32-bit wrap-around)
  {
    // the digits' first destinations: the exclusive scan of their totals
    uint64_t all;
    const uint64_t dbase = bk.exclusive((uint64_t)a.total[tid], (uint64_t)0, CutsAdd(), &all);
    uint32_t c = 0;
    for (uint32_t j = 0; j < (uint32_t)kWaves; ++j) {
      const uint32_t x = cnt[j * kCutsDigits + tid];
      cnt[j * kCutsDigits + tid] = c;
      c += x;
    }
    uint64_t tot;
    const uint32_t lb = (uint32_t)bk.exclusive((uint64_t)c, (uint64_t)0, CutsAdd(), &tot);
    for (uint32_t j = 0; j < (uint32_t)kWaves; ++j) cnt[j * kCutsDigits + tid] += lb;
    gdelta[tid] = (uint32_t)dbase + a.hist[(uint64_t)tid * a.ntiles + tile] - lb;
    if (tid == 0) gdelta[kCutsDigits] = (uint32_t)tot;
  }
  bk.sync();
  uint32_t *lcol = stage, *lkey = stage + kCutsTile;
#pragma unroll
  for (uint32_t r = 0; r < kCutsRounds; ++r) {
    if (!(tag[r] & 0x80000000u)) continue;
    const uint32_t i = wv * kCutsWaveRun + r * kWave + lane;
    const uint32_t d = (tag[r] >> 16) & (kCutsDigits - 1);
    const uint32_t at = cnt[wv * kCutsDigits + d] + (tag[r] & 0xFFFFu);  // (< the tile's kept entries)
    uint32_t col = 0, key = 0;
    if (kFirst) {  // (a kept entry: index < ncol)
      col = (uint32_t) static_cast<const IT *>(a.index)[k0 + i];
      key = w.has_val ? cuts_key(a.value[k0 + i]) : kCutsOneKey;
    } else {
      col = scol[i0 + i];
      key = skey[i0 + i];
    }
    lcol[at] = col;
    lkey[at] = key;
  }
  bk.sync();

  // the payload: (column, key) in runs of one digit, every destination below the kept count (<= max_entries)
  const uint32_t nk = gdelta[kCutsDigits];
  for (uint32_t j = tid; j < nk; j += kThreads) {
    const uint32_t col = lcol[j], key = lkey[j];
    const uint64_t dest = (uint32_t)(j + gdelta[cuts_digit(a.pass, col, key)]);
    if (dest < a.max_entries) {
      dcol[dest] = col;
      dkey[dest] = key;
    }
  }
}

// the first position in [lo, hi) of the ascending words s whose word is >= x (hi if none)
DA_HD uint64_t cuts_lower(const uint32_t *s, uint64_t lo, uint64_t hi, uint64_t x) {
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)s[mid] < x) lo = mid + 1;
    else hi = mid;
  }
  return lo;
}

// ---- bounds: cstart[c], c in 0 .. ncol, from the sorted columns
DA_HD void cuts_bounds(const CutsArgs &a, uint64_t c) {
  if (c > a.ncol || cuts_result_flags(a.res) != 0) return;
  a.cstart[c] = (uint32_t)cuts_lower(a.col[(a.passes - 1) & 1], 0, a.meta[CU_KEPT], c);
}

// rank pick i of a column of n samples at s: t[i] > t[i - 1] (i >= 1)
DA_HD bool cuts_pick(const uint32_t *s, uint64_t n, uint64_t B, uint64_t i, uint32_t *t) {
  *t = s[i * n / B];
  return *t > s[(i - 1) * n / B];
}

// ---- count: column c's samples, and its cuts to cut_ptr[c]
template <class BK>
DA_HDF void cuts_count_col(const CutsArgs &a, uint64_t c, BK &bk) {
  if (cuts_result_flags(a.res) != 0) return;  // (uniform)
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t *key = a.key[(a.passes - 1) & 1];
  const uint64_t lo = a.cstart[c], hi = a.cstart[c + 1];
  // the NaN keys stand last in the column
  uint64_t n = hi > lo ? hi - lo : 0;
  if (n != 0 && key[hi - 1] == kCutsNanKey) n = cuts_lower(key, lo, hi, kCutsNanKey) - lo;
  if (n == 0) {  // (uniform) no cuts
    if (tid == 0) a.cn[c] = a.cut_ptr[c] = 0;
    return;
  }
  const uint64_t B = a.max_bin;
  uint64_t mine = 0;
  for (uint64_t i = tid; i < B; i += kThreads) {
    uint32_t t;
    if (i >= 1 && cuts_pick(key + lo, n, B, i, &t)) ++mine;
  }
  uint64_t total;
  (void)bk.exclusive(mine, (uint64_t)0, CutsAdd(), &total);
  if (tid == 0) {
    a.cn[c] = (uint32_t)n;
    a.cut_ptr[c] = (uint32_t)total + 1;
  }
}

// ---- ptr: one workgroup scans cut_ptr in place and sets d_status
template <class BK>
DA_HDF void cuts_ptr(const CutsArgs &a, BK &bk) {
  const uint64_t sflags = cuts_result_flags(a.res);
  const uint32_t tid = (uint32_t)bk.tid();
  if (sflags != 0) {  // (uniform) no cuts, and the flags
    for (uint64_t c = tid; c <= a.ncol; c += kThreads) a.cut_ptr[c] = 0;
    if (tid == 0) {
      a.status[CU_KEPT] = 0;
      a.status[CU_DROPPED] = 0;
      a.status[CU_FIRST] = kNone;
      a.status[CU_FLAGS] = sflags;
      a.status[CU_NAN] = 0;
      a.status[CU_NCUTS] = 0;
      a.status[CU_EMPTY] = a.ncol;
      a.status[CU_ZERO] = 0;
    }
    return;
  }
  const uint64_t per = (a.ncol + kThreads - 1) / kThreads;
  const uint64_t c0 = mn<uint64_t>((uint64_t)tid * per, a.ncol), c1 = mn<uint64_t>(c0 + per, a.ncol);
  CutsSum mine = cuts_sum_zero();
  for (uint64_t c = c0; c < c1; ++c) {
    mine.cuts += a.cut_ptr[c];
    mine.n += a.cn[c];
    mine.empty += a.cut_ptr[c] == 0;
  }
  CutsSum all;
  const CutsSum ex = bk.exclusive(mine, cuts_sum_zero(), CutsSumAdd(), &all);
  uint64_t run = ex.cuts;
  for (uint64_t c = c0; c < c1; ++c) {
    const uint32_t m = a.cut_ptr[c];
    a.cut_ptr[c] = (uint32_t)run;
    run += m;
  }
  if (tid == 0) {
    a.cut_ptr[a.ncol] = (uint32_t)all.cuts;  // (< 2^32: ncol * max_bin is)
    const uint64_t kept = a.meta[CU_KEPT];
    a.status[CU_KEPT] = kept;
    a.status[CU_DROPPED] = a.meta[CU_DROPPED];
    a.status[CU_FIRST] = a.meta[CU_FIRST];
    a.status[CU_FLAGS] = a.meta[CU_FLAGS] | (all.cuts > a.cap ? (uint64_t)kCutsFlagCapacity : 0);
    a.status[CU_NAN] = kept - all.n;
    a.status[CU_NCUTS] = all.cuts;
    a.status[CU_EMPTY] = all.empty;
    a.status[CU_ZERO] = 0;
  }
}

// ---- write: column c's cuts to cut_value[cut_ptr[c] ..)
template <class BK>
DA_HDF void cuts_write_col(const CutsArgs &a, uint64_t c, BK &bk) {
  if (cuts_result_flags(a.res) != 0) return;  // (uniform)
  const uint64_t n = a.cn[c];
  if (n == 0) return;  // (uniform) no cuts
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t *s = a.key[(a.passes - 1) & 1] + a.cstart[c];
  const uint64_t B = a.max_bin;
  uint64_t run = a.cut_ptr[c];
  for (uint64_t base = 0; base < B; base += kThreads) {  // (uniform)
    const uint64_t i = base + tid;
    uint32_t t = 0;
    const bool keep = i >= 1 && i < B && cuts_pick(s, n, B, i, &t);
    uint64_t total;
    const uint64_t at = run + bk.exclusive((uint64_t)keep, (uint64_t)0, CutsAdd(), &total);
    if (keep && at < a.cap) a.cut_value[at] = cuts_unkey(t);
    run += total;
  }
  if (tid == 0 && run < a.cap) {  // just above the maximum
    const uint32_t top = s[n - 1];
    const uint32_t v = cuts_unkey(top == kCutsInfKey ? top : top + 1);
    a.cut_value[run] = v == 0x80000000u ? 0u : v;
  }
}

}  // namespace dmlc_amd
