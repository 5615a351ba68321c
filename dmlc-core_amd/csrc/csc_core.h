// csc_core.h -- CSC transpose of a parsed CSR (dmlc_amd_to_csc): the tile bodies.
// A stable counting sort of the window's entries by column, as an LSD radix
// sort over 8-bit digits of the column: P = ceil(bits(ncol - 1) / 8) passes of
// three plain launches each.  Tiles are kCscTile consecutive ENTRIES (not rows),
// so one row holding half of all entries is spread over every tile.
//   hist     one workgroup per tile: the tile's 256 digit counts (LDS atomics)
//            go to hist[digit][tile]; pass 0 reads `index` over the window's
//            entry range, counts only entries with index < ncol and stores the
//            tile's record {dropped, first dropped position, flags}
//   scan     256 workgroups, one per digit: the exclusive scan of the digit's
//            row of tile counts in place, and the digit's total.  After pass 0
//            workgroup 0 also sums the records and sets d_status
//   scatter  one workgroup per tile: re-reads the keys, ranks them stably and
//            moves the payload.  A tile's entries are ordered wave, round, lane;
//            in a round a lane finds the lanes of its wave with the same digit
//            by eight ballots, its rank is the wave's running count of the
//            digit (LDS) plus the matching lower lanes, and the group's first
//            lane adds the group's size.  The waves' counts are then scanned
//            per digit on top of (digit base + the tile's scanned count).
//            Pass 0 finds each entry's row in the offsets the tile spans
//            (staged in LDS when they fit); the last pass stores row / value /
//            pos, every store checked against the capacity; passes between
//            carry (column, row, value bits, relative position) through two
//            workspace buffers.
//   bounds   (P > 1) col_offset[c] = the first sorted entry with column >= c,
//            one thread per word.  With one pass the digit totals are the
//            column counts and the scatter's first tile stores col_offset.
// Dropped entries are counted in the tile records, not by atomics on d_status:
// the status would have to be zeroed by an earlier launch, and a record per
// tile keeps the count and the first position deterministic (as gather_core.h).
// No workgroup waits for another.  Everything moves as bit patterns (IT / VT =
// uint32_t or uint64_t).  Compiles as HIP device code (block.h) and as plain
// C++ with a host block (tests/emu/csc_check.cpp).
#pragma once
#include "common.h"

namespace dmlc_amd {

#ifndef DMLC_AMD_CSC_ROUNDS
#define DMLC_AMD_CSC_ROUNDS 16
#endif
constexpr uint32_t kCscRounds = DMLC_AMD_CSC_ROUNDS;     // entries per thread
constexpr uint32_t kCscTile = kThreads * kCscRounds;     // entries per tile
constexpr uint32_t kCscWaveRun = kWave * kCscRounds;     // consecutive entries of one wave
constexpr uint32_t kCscRadixBits = 8;
constexpr uint32_t kCscDigits = 1u << kCscRadixBits;     // == kThreads: one digit per thread / scan workgroup
constexpr uint32_t kCscSpan = kCscTile + 63;             // most rows whose offsets a tile stages in LDS
constexpr uint32_t kCscRecWords = 4;                     // workspace words per tile record
constexpr uint64_t kCscMaxWindow = 0xFFFFFFFFull;        // a window of this many rows or entries is refused
static_assert(kCscDigits == (uint32_t)kThreads, "one digit per thread");
static_assert(kCscWaveRun <= 0x10000u, "a wave-local rank fits 16 bits");

// d_status words and flag bits (include/dmlc_amd.h)
enum { CS_KEPT = 0, CS_DROPPED = 1, CS_FIRST = 2, CS_FLAGS = 3 };
enum {
  kCscFlagError = 1u,
  kCscFlagValueCount = 2u,
  kCscFlagOffsetCap = 4u,
  kCscFlagCapacity = 8u,
  kCscFlagMaxEntries = 16u
};

// the carried payload of the passes between the first and the last
struct CscBuf {
  uint32_t *col, *row, *rpos;
  void *val;
};

struct CscArgs {
  const uint64_t *offset;
  const void *index;
  const void *value;
  const uint64_t *res;  // the source's device result block (dmlc_amd_result)
  uint64_t cap_rows, cap_index, cap_value;
  uint64_t row_begin, row_end;  // the row window (row_end saturates)
  uint64_t ncol;
  uint64_t max_entries;  // the launches are sized for this many entries
  uint64_t ntiles;       // tiles launched, and the stride of hist's digit rows
  uint32_t passes, pass;
  // outputs
  uint64_t *col_offset;
  uint32_t *row;
  void *val;
  uint64_t *pos;
  uint64_t cap;
  uint64_t *status;
  // workspace
  uint64_t *meta;   // [0] = kept (set by the scan of pass 0)
  uint32_t *total;  // kCscDigits digit totals of the current pass
  uint64_t *rec;    // ntiles records of kCscRecWords words
  uint32_t *hist;   // kCscDigits rows of ntiles counts
  CscBuf buf[2];
};

// digit passes for ncol columns
DA_HD uint32_t csc_passes(uint64_t ncol) {
  uint32_t p = 1;
  for (uint64_t m = (ncol - 1) >> kCscRadixBits; m != 0; m >>= kCscRadixBits) ++p;
  return p;
}

// flag bits 0 and 1: the parse failed, or its value count fits no RowBlock;
// nothing is written then (every col_offset word is still set to 0)
DA_HD uint64_t csc_result_flags(const uint64_t *res) {
  uint64_t f = 0;
  if (res[8] != 0) f |= kCscFlagError;
  if (res[C_VALUE] != 0 && res[C_VALUE] != res[C_INDEX]) f |= kCscFlagValueCount;
  return f;
}

// the window: its rows [r0, r1), its entries [e0, e0 + E), no source element at
// or past lim is read
struct CscWin {
  uint64_t r0, r1, e0, E, lim, flags;
  bool has_val;
};
DA_HD CscWin csc_window(const CscArgs &a) {
  CscWin w;
  w.has_val = a.res[C_VALUE] != 0;
  w.lim = w.has_val ? mn<uint64_t>(a.cap_index, a.cap_value) : a.cap_index;
  w.flags = 0;
  w.r0 = a.row_begin;
  w.r1 = mn<uint64_t>(mn<uint64_t>(a.res[C_ROWS], a.cap_rows), a.row_end);
  w.e0 = w.E = 0;
  if (w.r1 <= w.r0) {  // an empty window
    w.r1 = w.r0;
    return w;
  }
  uint64_t o0 = a.offset[w.r0], o1 = a.offset[w.r1];
  if (o0 > w.lim || o1 > w.lim) {
    o0 = mn<uint64_t>(o0, w.lim);
    o1 = mn<uint64_t>(o1, w.lim);
    w.flags |= kCscFlagOffsetCap;
  }
  w.e0 = o0;
  w.E = o1 > o0 ? o1 - o0 : 0;  // (descending offsets: nothing is read)
  if (w.E > a.max_entries) {    // the launches hold no more
    w.E = a.max_entries;
    w.flags |= kCscFlagMaxEntries;
  }
  return w;
}

// entries the current pass sorts: the window's in pass 0, the kept ones after it
DA_HD uint64_t csc_pass_entries(const CscArgs &a, const CscWin &w) { return a.pass == 0 ? w.E : a.meta[0]; }

// offset[j] clamped; the last row j in [lo, hi) with offset[j] <= k (lo if none)
DA_HD uint64_t csc_off(const CscArgs &a, const CscWin &w, uint64_t j) { return mn<uint64_t>(a.offset[j], w.lim); }
DA_HD uint64_t csc_row_of(const CscArgs &a, const CscWin &w, uint64_t k, uint64_t lo, uint64_t hi) {
  while (hi - lo > 1) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if (csc_off(a, w, mid) <= k) lo = mid;
    else hi = mid;
  }
  return lo;
}

struct CscRec {
  uint64_t dropped, first;
};
struct CscRecAdd {
  DA_HD CscRec operator()(const CscRec &x, const CscRec &y) const {
    CscRec r;
    r.dropped = x.dropped + y.dropped;
    r.first = mn<uint64_t>(x.first, y.first);
    return r;
  }
};
DA_HD CscRec csc_rec_zero() {
  CscRec z;
  z.dropped = 0;
  z.first = kNone;
  return z;
}
struct CscAdd {
  DA_HD uint64_t operator()(uint64_t x, uint64_t y) const { return x + y; }
};

// ---- hist.  cnt: kCscDigits words
template <typename IT, class BK>
DA_HDF void csc_hist_tile(const CscArgs &a, uint64_t tile, uint32_t *cnt, BK &bk) {
  if (csc_result_flags(a.res) != 0) return;  // (uniform) the scan does not read the counts then
  const CscWin w = csc_window(a);
  const uint64_t n = csc_pass_entries(a, w);
  const uint64_t i0 = tile * kCscTile;
  if (i0 >= n) return;  // (uniform) past the real count: the scan reads ceil(n / tile) tiles
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t nl = (uint32_t)mn<uint64_t>(kCscTile, n - i0);
  const uint32_t shift = a.pass * kCscRadixBits;
  cnt[tid] = 0;
  bk.sync();
  CscRec mine = csc_rec_zero();
  if (a.pass == 0) {
    const IT *index = static_cast<const IT *>(a.index) + w.e0 + i0;
    for (uint32_t i = tid; i < nl; i += kThreads) {
      const uint64_t c = (uint64_t)index[i];
      if (c >= a.ncol) {
        ++mine.dropped;
        mine.first = mn<uint64_t>(mine.first, w.e0 + i0 + i);
      } else {
        (void)atomic_add_u32(&cnt[(uint32_t)c & (kCscDigits - 1)], 1u);
      }
    }
  } else {
    const uint32_t *col = a.buf[(a.pass - 1) & 1].col + i0;
    for (uint32_t i = tid; i < nl; i += kThreads) (void)atomic_add_u32(&cnt[(col[i] >> shift) & (kCscDigits - 1)], 1u);
  }
  bk.sync();
  a.hist[(uint64_t)tid * a.ntiles + tile] = cnt[tid];
  if (a.pass == 0) {
    CscRec total;
    (void)bk.exclusive(mine, csc_rec_zero(), CscRecAdd(), &total);
    if (tid == 0) {
      uint64_t *rec = a.rec + tile * kCscRecWords;
      rec[0] = total.dropped;
      rec[1] = total.first;
      rec[2] = w.flags;
      rec[3] = 0;
    }
  }
}

// ---- scan: workgroup `digit` scans hist[digit][0 .. tiles) in place
template <class BK>
DA_HDF void csc_scan(const CscArgs &a, uint32_t digit, BK &bk) {
  const uint64_t sflags = csc_result_flags(a.res);
  const uint32_t tid = (uint32_t)bk.tid();
  if (sflags != 0) {  // (uniform) nothing is transposed: an empty CSC and the flags
    if (a.pass != 0) return;
    for (uint64_t c = (uint64_t)digit * kThreads + tid; c <= a.ncol; c += (uint64_t)kCscDigits * kThreads) a.col_offset[c] = 0;
    if (digit == 0 && tid == 0) {
      a.status[CS_KEPT] = 0;
      a.status[CS_DROPPED] = 0;
      a.status[CS_FIRST] = kNone;
      a.status[CS_FLAGS] = sflags;
      a.meta[0] = 0;
    }
    return;
  }
  const CscWin w = csc_window(a);
  const uint64_t n = csc_pass_entries(a, w);
  const uint64_t nt = n / kCscTile + (n % kCscTile != 0);  // (<= a.ntiles: n <= max_entries)
  const uint64_t per = (nt + kThreads - 1) / kThreads;
  const uint64_t t0 = mn<uint64_t>((uint64_t)tid * per, nt), t1 = mn<uint64_t>(t0 + per, nt);
  uint32_t *h = a.hist + (uint64_t)digit * a.ntiles;
  uint64_t mine = 0;
  for (uint64_t k = t0; k < t1; ++k) mine += h[k];
  uint64_t total;
  uint64_t run = bk.exclusive(mine, (uint64_t)0, CscAdd(), &total);
  for (uint64_t k = t0; k < t1; ++k) {
    const uint32_t c = h[k];
    h[k] = (uint32_t)run;
    run += c;
  }
  if (tid == 0) a.total[digit] = (uint32_t)total;
  if (a.pass != 0 || digit != 0) return;  // (uniform)
  // the status: the records' sums
  CscRec r = csc_rec_zero();
  for (uint64_t k = t0; k < t1; ++k) {
    CscRec x;
    x.dropped = a.rec[k * kCscRecWords];
    x.first = a.rec[k * kCscRecWords + 1];
    r = CscRecAdd()(r, x);
  }
  CscRec all;
  (void)bk.exclusive(r, csc_rec_zero(), CscRecAdd(), &all);
  if (tid == 0) {
    const uint64_t kept = w.E - all.dropped;
    a.status[CS_KEPT] = kept;
    a.status[CS_DROPPED] = all.dropped;
    a.status[CS_FIRST] = all.first;
    a.status[CS_FLAGS] = w.flags | (kept > a.cap ? (uint64_t)kCscFlagCapacity : 0);
    a.meta[0] = kept;
  }
}

// ---- scatter.  cnt: kWaves * kCscDigits words; span: kCscSpan + 1 words;
// ends: 2 words
template <typename IT, typename VT, class BK>
DA_HDF void csc_scatter_tile(const CscArgs &a, uint64_t tile, uint32_t *cnt, uint32_t *span, uint64_t *ends, BK &bk) {
  if (csc_result_flags(a.res) != 0) return;  // (the scan of pass 0 zeroed col_offset)
  const CscWin w = csc_window(a);
  const uint64_t n = csc_pass_entries(a, w);
  const uint32_t tid = (uint32_t)bk.tid();
  const uint32_t lane = tid & (kWave - 1), wv = tid / kWave;
  const bool last = a.pass + 1 == a.passes;
  const uint32_t shift = a.pass * kCscRadixBits;

  // the digits' first destinations: the exclusive scan of their totals
  uint64_t all;
  const uint64_t dbase = bk.exclusive((uint64_t)a.total[tid], (uint64_t)0, CscAdd(), &all);
  if (a.passes == 1 && tile == 0) {  // one pass: the digit totals are the column counts
    if (tid < a.ncol) a.col_offset[tid] = dbase;
    if (tid == 0) a.col_offset[a.ncol] = all;
  }
  const uint64_t i0 = tile * kCscTile;
  if (i0 >= n) return;  // (uniform) past the real count
  const uint32_t nl = (uint32_t)mn<uint64_t>(kCscTile, n - i0);
  for (uint32_t j = 0; j < (uint32_t)kWaves; ++j) cnt[j * kCscDigits + tid] = 0;

  const IT *index = static_cast<const IT *>(a.index);
  const CscBuf src = a.buf[(a.pass + 1) & 1];  // (pass > 0: what pass - 1 wrote)
  const CscBuf dst = a.buf[a.pass & 1];
  const uint64_t k0 = w.e0 + i0;  // pass 0: the tile's first source position

  // pass 0: the rows of the tile's first and last entry, and their offsets
  uint64_t ra = 0, rb = 0;
  uint32_t nspan = 0;
  bool staged = false;
  if (a.pass == 0) {
    if (tid == 0) ends[0] = csc_row_of(a, w, k0, w.r0, w.r1);
    if (tid == (uint32_t)kWave) ends[1] = csc_row_of(a, w, k0 + nl - 1, w.r0, w.r1);
    bk.sync();
    ra = ends[0];
    rb = mx<uint64_t>(ends[1], ra);
    staged = rb - ra < (uint64_t)kCscSpan;
    nspan = staged ? (uint32_t)(rb - ra) + 1 : 0;
    if (staged)
      for (uint32_t j = tid; j <= nspan; j += kThreads) span[j] = (uint32_t)(csc_off(a, w, ra + j) - w.e0);
  }
  bk.sync();

  // ranks: tag = valid | digit << 16 | rank among the wave's earlier entries of the digit
  uint32_t tag[kCscRounds];
#pragma unroll
  for (uint32_t r = 0; r < kCscRounds; ++r) {
    const uint32_t i = wv * kCscWaveRun + r * kWave + lane;
    bool valid = i < nl;
    uint32_t c = 0;
    if (valid) {
      if (a.pass == 0) {
        const uint64_t c64 = (uint64_t)index[k0 + i];
        valid = c64 < a.ncol;
        c = (uint32_t)c64;
      } else {
        c = src.col[i0 + i];
      }
    }
    const uint32_t d = (c >> shift) & (kCscDigits - 1);
    uint64_t peers = bk.ballot(valid);
#pragma unroll
    for (uint32_t b = 0; b < kCscRadixBits; ++b) {
      const bool bit = (d >> b) & 1u;
      const uint64_t m = bk.ballot(bit);
      peers &= bit ? m : ~m;
    }
    const uint32_t below = (uint32_t)popc64(peers & ((1ull << lane) - 1));
    uint32_t *slot = &cnt[wv * kCscDigits + d];
    const uint32_t prev = valid ? *slot : 0;
    bk.wave_sync();
    if (valid && below == 0) *slot = prev + (uint32_t)popc64(peers);
    bk.wave_sync();
    tag[r] = valid ? (0x80000000u | (d << 16) | (prev + below)) : 0u;
  }
  bk.sync();

  // the waves' counts, scanned per digit on top of the tile's first destination
  {
    uint32_t g = (uint32_t)dbase + a.hist[(uint64_t)tid * a.ntiles + tile];
    for (uint32_t j = 0; j < (uint32_t)kWaves; ++j) {
      const uint32_t c = cnt[j * kCscDigits + tid];
      cnt[j * kCscDigits + tid] = g;
      g += c;
    }
  }
  bk.sync();

  // the payload
  const VT *svalue = static_cast<const VT *>(a.value);
  const bool move_val = w.has_val && a.val != nullptr;
  const bool move_pos = a.pos != nullptr;
  const float scale = a.pass == 0 ? (float)nspan / (float)nl : 0.f;
#pragma unroll
  for (uint32_t r = 0; r < kCscRounds; ++r) {
    if (!(tag[r] & 0x80000000u)) continue;
    const uint32_t i = wv * kCscWaveRun + r * kWave + lane;
    const uint32_t d = (tag[r] >> 16) & (kCscDigits - 1);
    const uint64_t dest = (uint64_t)cnt[wv * kCscDigits + d] + (tag[r] & 0xFFFFu);
    uint32_t col, row, rpos;
    VT v = 0;
    if (a.pass == 0) {
      const uint64_t k = k0 + i;
      col = (uint32_t)index[k];
      rpos = (uint32_t)(i0 + i);
      if (move_val) v = svalue[k];  // (k < lim: the window's clamped range)
      // the entry's row: the last j with offset[j] <= k (empty rows share an
      // offset with their successor); a first guess, then a binary search
      uint64_t rr;
      if (staged) {
        const uint32_t rel = rpos;
        uint32_t gs = (uint32_t)((float)i * scale);
        gs = gs < nspan ? gs : nspan - 1;
        uint32_t lo, hi;
        if (span[gs] <= rel) {
          lo = gs;
          hi = span[gs + 1] > rel ? gs + 1 : nspan;
        } else {
          lo = 0;
          hi = gs;
        }
        while (hi - lo > 1) {
          const uint32_t mid = (lo + hi) >> 1;
          if (span[mid] <= rel) lo = mid;
          else hi = mid;
        }
        rr = ra + lo;
      } else {
        rr = csc_row_of(a, w, k, ra, rb + 1);
      }
      row = (uint32_t)(rr - w.r0);
    } else {
      const uint64_t s = i0 + i;
      col = src.col[s];
      row = src.row[s];
      rpos = move_pos ? src.rpos[s] : 0;
      if (move_val) v = static_cast<const VT *>(src.val)[s];
    }
    if (last) {
      if (a.passes > 1) dst.col[dest] = col;  // the sorted columns: bounds reads them
      if (dest < a.cap) {
        a.row[dest] = row;
        if (move_val) static_cast<VT *>(a.val)[dest] = v;
        if (move_pos) a.pos[dest] = w.e0 + rpos;
      }
    } else {
      dst.col[dest] = col;
      dst.row[dest] = row;
      if (move_pos) dst.rpos[dest] = rpos;
      if (move_val) static_cast<VT *>(dst.val)[dest] = v;
    }
  }
}

// ---- bounds (passes > 1): col_offset[c], c in 0 .. ncol, from the sorted columns
DA_HD void csc_bounds(const CscArgs &a, uint64_t c) {
  if (c > a.ncol || csc_result_flags(a.res) != 0) return;
  const uint32_t *col = a.buf[(a.passes - 1) & 1].col;
  uint64_t lo = 0, hi = a.meta[0];  // the first entry with column >= c
  while (lo < hi) {
    const uint64_t mid = lo + ((hi - lo) >> 1);
    if ((uint64_t)col[mid] < c) lo = mid + 1;
    else hi = mid;
  }
  a.col_offset[c] = lo;
}

}  // namespace dmlc_amd
