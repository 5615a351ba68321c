// bins_core.h -- CSR -> quantised dense row batch (dmlc_amd_to_bins): the tile body.
//
// The tile, its LDS tags and its first two phases are dense_core.h's: a
// 256-thread workgroup owns nr rows x ns columns (dense_shape), and after
//   A  zero the tags, load the offsets; here also the tile's ns + 1 cut_ptr
//      words go to LDS (every row of the tile reads them again)
//   B  per entry, an LDS max of (position in the row) + 1 into its cell
// every cell's tag names its winning entry.  (A and B are restated here, not
// shared: factoring them out of dense_tile changed dense_tile_kernel's
// register allocation.)  Then
//   B' (with B, before its barrier) the tile's columns: the largest usable cut
//      count m_max -- it fixes the depth of the search for the whole tile --
//      and whether cut_ptr ascends over the tile's columns
//   C  every cell's owner loads the winning value and runs the branch-free
//      upper-bound search over its column's cuts: pos = #{cuts <= v}, found
//      by depth = bit_width(m_max) steps "pos += step if pos + step <= m and
//      cut[pos + step - 1] <= v" -- one dependent load per step.  Where the
//      loads go is decided per tile (uniformly):
//        staged  the tile walks its columns in groups of G = kBinsLdsCuts /
//                m_max; a group's cuts (one ascending range of cut_value, at
//                most kBinsLdsCuts floats) are copied to LDS by coalesced
//                loads, then the group's nr x G cells are searched there.
//                Every cut of the tile's columns is read once per tile.
//        global  the search reads cut_value itself (L1 / L2): each step of
//                each cell fetches a cache line for one float, so this pays
//                only where the cells with an entry are few beside the cuts
//                (sparse wide rows), or where the cuts cannot be staged
//                (cut_ptr descends somewhere, a column of more than
//                kBinsLdsCuts cuts).
//      The rule: staged when 4 bytes x the tile's cuts <= 64 bytes x depth x
//      the tile's entries.  A thread runs several cells' searches side by
//      side (independent chains).  The code replaces the cell's tag.
//   D  the codes leave LDS packed: a tile that is one contiguous span of
//      `out` (ld == ncol, no column tiling) stores 16 bytes per lane apart
//      from an unaligned head and tail; otherwise per element.
// The NaN / unbinned counts and the new flag bits are summed in LDS and reach
// d_status by at most one global atomic each per tile, only when non-zero.
// No workgroup talks to another.  Compiles as HIP device code (block.h) and
// as plain C++ with a host block (tests/emu/bins_check.cpp).
#pragma once
#include "dense_core.h"

namespace dmlc_amd {

constexpr uint32_t kBinsLdsCuts = 4096;  // cut values a column group stages in LDS (floats)
constexpr int kBinsUnrollLds = 4;        // searches a thread runs side by side over staged cuts (a group of more
                                         // than kThreads cells; a smaller one gives a thread one cell, one search)
constexpr int kBinsUnrollGlobal = 8;     // ... over cut_value in global memory
constexpr uint64_t kBinsLineBytes = 64;  // what a search step in global memory is charged (the staging rule)

// d_status words past the dense ones, and the flag bits past the dense ones
enum { BS_NAN = 4, BS_UNBINNED = 5, BS_WORDS = 8 };
enum { kBinsFlagCodeRange = 16u, kBinsFlagCutPtr = 32u };
// the tile's small LDS words
enum { BL_BAD = 0, BL_FLAGS, BL_NAN, BL_UNBINNED, BL_MMAX, BL_DESCENDS, BL_PATH, BL_WORDS = 8 };
// BL_PATH: where the tile's searches read.  Test-only: tests/emu/bins_check.cpp reads it after the tile to
// assert that each path ran; on the device it is one LDS store a tile that nothing reads.
enum { kBinsPathStaged = 1u, kBinsPathGlobal = 2u, kBinsPathStagedGroups = 3u /* staged, several column groups */ };

struct BinsArgs {
  DenseArgs d;  // the window, the tile shape, out and status (fill is unused; one = 1.0f)
  const uint32_t *cut_ptr;
  const float *cut_value;
  uint64_t n_cuts;
  uint32_t missing;     // the code of a cell without a usable value
  uint32_t global_ids;  // DMLC_AMD_BINS_GLOBAL: cut_ptr[c] is added to the code
};

// d_status before the tiles run (one thread)
DA_HD void bins_status_init(const BinsArgs &b) {
  dense_status_init(b.d);
  for (int i = BS_NAN; i < BS_WORDS; ++i) b.d.status[i] = 0;
}

template <typename CT>
struct alignas(16) BinsVec {
  CT v[16 / sizeof(CT)];
};

// One thread's cells q0, q0 + kThreads, ... (U of them) of the nr x gn cells of the column group that starts at
// tile column g0 (the whole tile: g0 = 0, gn = ns): value, cuts, search, code -> tags.
// cv[i - sub] is cut_value[i] (cv: the LDS copy, or cut_value itself with sub == 0).
template <typename CT, int U>
DA_HDF void bins_cells(const BinsArgs &b, const float *cv, uint32_t sub, uint32_t depth, uint32_t q0, uint32_t nq,
                       uint32_t gn, uint32_t g0, uint32_t ns, uint64_t lim, bool has_val, uint32_t *tags,
                       const uint64_t *offs, const uint32_t *cptr, uint32_t *flags, uint32_t *n_nan, uint32_t *n_unb) {
  const float *value = static_cast<const float *>(b.d.value);
  constexpr uint64_t kMaxCode = sizeof(CT) == 1 ? 0xFFull : sizeof(CT) == 2 ? 0xFFFFull : 0xFFFFFFFFull;
  float v[U];
  uint32_t cell[U], lo[U], base[U], m[U], pos[U];
  bool binned[U];
#pragma unroll
  for (int i = 0; i < U; ++i) {
    const uint32_t q = q0 + (uint32_t)i * kThreads;
    v[i] = 0.0f;
    cell[i] = lo[i] = base[i] = m[i] = pos[i] = 0;
    binned[i] = false;
    if (q >= nq) continue;
    const uint32_t row = q / gn, col = g0 + (q - row * gn);
    const uint32_t j = row * ns + col;
    cell[i] = j;
    const uint32_t tag = tags[j];
    if (tag == 0) continue;  // no entry
    float x = u2f((uint32_t)b.d.one);  // RowBlock::get_value: no value array means 1
    if (has_val) {
      const uint64_t k = offs[row] + tag - 1;
      if (k >= lim) continue;  // (k < lim always, for ascending offsets)
      x = value[k];
    }
    const uint32_t cb = cptr[col], ce = cptr[col + 1];
    const bool usable = cb <= ce && (uint64_t)ce <= b.n_cuts;
    if (!usable) *flags |= kBinsFlagCutPtr;
    if (!usable || ce == cb) {
      ++*n_unb;
    } else if (x != x) {
      ++*n_nan;
    } else {
      v[i] = x;
      lo[i] = cb;
      base[i] = cb - sub;
      m[i] = ce - cb;  // no cut at or past cb + m <= n_cuts is read
      binned[i] = true;
    }
  }
  for (uint32_t step = depth ? 1u << (depth - 1) : 0; step != 0; step >>= 1) {
#pragma unroll
    for (int i = 0; i < U; ++i) {
      // every lane loads, none branches: a cell that has nothing to search (m == 0) or whose column is
      // exhausted (t > m) reads an element that exists -- cv[0] (global memory: depth > 0, so some column holds
      // a cut; LDS: word 0 of lcut, which a group without cuts sets to 0 before the searches), or its
      // column's last cut -- and drops it
      const uint32_t t = pos[i] + step, tt = mn<uint32_t>(t, m[i]);
      const float c = cv[base[i] + (tt ? tt - 1 : 0u)];
      pos[i] = ((t <= m[i]) & (c <= v[i])) ? t : pos[i];
    }
  }
#pragma unroll
  for (int i = 0; i < U; ++i) {
    if (q0 + (uint32_t)i * kThreads >= nq) continue;
    uint32_t code = b.missing;
    if (binned[i]) {
      // the upper bound clamped to the last bin (HistogramCuts::SearchBin)
      const uint64_t c = (uint64_t)mn<uint32_t>(pos[i], m[i] - 1) + (b.global_ids ? lo[i] : 0u);
      if (c > kMaxCode || c == b.missing) *flags |= kBinsFlagCodeRange;
      else code = (uint32_t)c;
    }
    tags[cell[i]] = code;
  }
}

// tags: kDenseCells words, 16-byte aligned; offs: kDenseRows + 1; cptr: kDenseCells + 1;
// lcut: kBinsLdsCuts; sm: BL_WORDS
template <typename IT, typename CT, class BK>
DA_HDF void bins_tile(const BinsArgs &b, uint64_t tile, uint32_t *tags, uint64_t *offs, uint32_t *cptr, float *lcut,
                      uint32_t *sm, BK &bk) {
  const DenseArgs &a = b.d;
  if (dense_result_flags(a.res) != 0) return;
  const uint64_t rend = dense_row_end(a);
  const uint64_t trow = tile / a.col_tiles;
  const uint32_t tcol = (uint32_t)(tile % a.col_tiles);
  const uint64_t r0 = a.row_begin + trow * a.R;
  if (r0 >= rend) return;  // rows the parse did not produce: never written
  const uint32_t nr = (uint32_t)mn<uint64_t>(a.R, rend - r0);
  const uint64_t c0 = (uint64_t)tcol * a.S;
  const uint32_t ns = (uint32_t)mn<uint64_t>(a.S, a.ncol - c0);
  const uint32_t ncell = nr * ns;
  const bool has_val = a.res[C_VALUE] != 0;
  // no index / value element at or past the capacity is read
  const uint64_t lim = has_val ? mn<uint64_t>(a.cap_index, a.cap_value) : a.cap_index;
  const uint32_t tid = (uint32_t)bk.tid();

  // ---- A (dense_core.h), and the tile's cut_ptr words
  {
    DenseTag4 z;
    z.t[0] = z.t[1] = z.t[2] = z.t[3] = 0;
    DenseTag4 *t4 = reinterpret_cast<DenseTag4 *>(tags);
    for (uint32_t j = tid; j < (ncell + 3) / 4; j += kThreads) t4[j] = z;
    for (uint32_t j = tid; j <= nr; j += kThreads) {
      uint64_t o = a.offset[r0 + j];
      if (o > lim) {
        o = lim;
        atomic_or_u64(&a.status[DS_FLAGS], kDenseFlagOffsetCap);
      }
      offs[j] = o;
    }
    for (uint32_t j = tid; j <= ns; j += kThreads) cptr[j] = b.cut_ptr[c0 + j];
    if (tid < BL_WORDS) sm[tid] = 0;
  }
  bk.sync();
  const uint64_t e0 = offs[0], e1 = offs[nr];
  if (e1 - e0 >= kDenseMaxRowLen) {  // (uniform) some row may not fit the tag: look at each
    for (uint32_t j = tid; j < nr; j += kThreads)
      if (offs[j + 1] - offs[j] >= kDenseMaxRowLen) atomic_or_u32(&sm[BL_BAD], 1u);
    bk.sync();
    if (sm[BL_BAD] != 0) {  // refused: the flag, and nothing of this tile is written
      if (tid == 0) atomic_or_u64(&a.status[DS_FLAGS], kDenseFlagRowTooLong);
      return;
    }
  }

  // ---- B (dense_core.h)
  if (e1 > e0) {
    const IT *index = static_cast<const IT *>(a.index);
    const float scale = (float)nr / (float)(e1 - e0);
    uint64_t dropped = 0, first = kNone;
    for (uint64_t k = e0 + tid; k < e1; k += kThreads) {
      uint32_t g = (uint32_t)((float)(k - e0) * scale);
      g = g < nr ? g : nr - 1;
      uint32_t lo, hi;
      if (offs[g] <= k) {
        lo = g;
        hi = offs[g + 1] > k ? g + 1 : nr;
      } else {
        lo = 0;
        hi = g;
      }
      while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (offs[mid] <= k) lo = mid;
        else hi = mid;
      }
      const uint64_t c = (uint64_t)index[k];
      if (c >= a.ncol) {
        if (tcol == 0) {  // every column tile walks these entries: one counts them
          ++dropped;
          first = mn<uint64_t>(first, k);
        }
      } else if (c - c0 < (uint64_t)ns) {
        atomic_max_u32(&tags[lo * ns + (uint32_t)(c - c0)], (uint32_t)(k - offs[lo]) + 1u);
      }
    }
    if (dropped != 0) {
      atomic_add_u64(&a.status[DS_DROPPED], dropped);
      atomic_min_u64((unsigned long long *)&a.status[DS_FIRST], (unsigned long long)first);
    }
  }
  // ---- B': the columns' cut counts, and whether cut_ptr ascends over them
  {
    uint32_t mmax = 0, descends = 0;
    for (uint32_t j = tid; j < ns; j += kThreads) {
      const uint32_t cb = cptr[j], ce = cptr[j + 1];
      if (cb > ce) descends = 1;
      else if ((uint64_t)ce <= b.n_cuts) mmax = mx<uint32_t>(mmax, ce - cb);
    }
    if (mmax != 0) atomic_max_u32(&sm[BL_MMAX], mmax);
    if (descends != 0) atomic_or_u32(&sm[BL_DESCENDS], 1u);
  }
  bk.sync();
  const uint32_t mmax = sm[BL_MMAX];
  const uint32_t depth = mmax ? 32u - (uint32_t)clz32(mmax) : 0u;
  // (uniform) ascending cut_ptr inside the capacity: every column is usable, holds at most mmax cuts, and a run
  // of columns owns one range of cut_value
  const uint32_t lo_all = cptr[0], hi_all = cptr[ns];
  const bool staged = sm[BL_DESCENDS] == 0 && (uint64_t)hi_all <= b.n_cuts && mmax != 0 && mmax <= kBinsLdsCuts &&
                      4ull * (hi_all - lo_all) <= kBinsLineBytes * depth * (e1 - e0);

  // ---- C
  uint32_t flags = 0, n_nan = 0, n_unb = 0;
  if (staged) {
    const uint32_t G = kBinsLdsCuts / mmax;  // columns a group
    for (uint32_t g0 = 0; g0 < ns; g0 += G) {
      const uint32_t gn = mn<uint32_t>(G, ns - g0), lo = cptr[g0];
      const uint32_t n = mn<uint32_t>(cptr[g0 + gn] - lo, kBinsLdsCuts);  // (<= gn * mmax: the bound never cuts)
      if (g0 != 0) bk.sync();  // the last group's searches are done with lcut
      for (uint32_t j = tid; j < n; j += kThreads) lcut[j] = b.cut_value[lo + j];
      if (n == 0 && tid == 0) lcut[0] = 0.0f;  // the word a cell without cuts reads and drops
      bk.sync();
      const uint32_t nq = nr * gn;
      if (nq <= (uint32_t)kThreads) {  // (uniform) one cell a thread: no idle chains beside it
        if (tid < nq)
          bins_cells<CT, 1>(b, lcut, lo, depth, tid, nq, gn, g0, ns, lim, has_val, tags, offs, cptr, &flags, &n_nan, &n_unb);
      } else {
        for (uint32_t q0 = tid; q0 < nq; q0 += kBinsUnrollLds * kThreads)
          bins_cells<CT, kBinsUnrollLds>(b, lcut, lo, depth, q0, nq, gn, g0, ns, lim, has_val, tags, offs, cptr, &flags,
                                         &n_nan, &n_unb);
      }
    }
  } else {
    for (uint32_t q0 = tid; q0 < ncell; q0 += kBinsUnrollGlobal * kThreads)
      bins_cells<CT, kBinsUnrollGlobal>(b, b.cut_value, 0u, depth, q0, ncell, ns, 0u, ns, lim, has_val, tags, offs, cptr,
                                        &flags, &n_nan, &n_unb);
  }
  if (flags != 0) atomic_or_u32(&sm[BL_FLAGS], flags);
  if (n_nan != 0) atomic_add_u32(&sm[BL_NAN], n_nan);
  if (n_unb != 0) atomic_add_u32(&sm[BL_UNBINNED], n_unb);
  bk.sync();
  if (tid == 0) {  // one global atomic per tile and word, when there is something to say
    if (sm[BL_FLAGS] != 0) atomic_or_u64(&a.status[DS_FLAGS], sm[BL_FLAGS]);
    if (sm[BL_NAN] != 0) atomic_add_u64(&a.status[BS_NAN], sm[BL_NAN]);
    if (sm[BL_UNBINNED] != 0) atomic_add_u64(&a.status[BS_UNBINNED], sm[BL_UNBINNED]);
    sm[BL_PATH] = !staged ? kBinsPathGlobal : (kBinsLdsCuts / mmax < ns ? kBinsPathStagedGroups : kBinsPathStaged);
  }

  // ---- D
  CT *out = static_cast<CT *>(a.out);
  const uint64_t row0 = r0 - a.row_begin;
  if (a.ld == a.ncol && a.col_tiles == 1) {
    // one contiguous span of ncell elements
    constexpr uint32_t V = 16 / sizeof(CT);
    CT *p = out + row0 * a.ld;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint32_t head = mn<uint32_t>(ncell, ((16u - mis) & 15u) / (uint32_t)sizeof(CT));
    const uint32_t ngroup = (ncell - head) / V;
    const uint32_t tail0 = head + ngroup * V;
    if (tid < head) p[tid] = (CT)tags[tid];
    for (uint32_t gidx = tid; gidx < ngroup; gidx += kThreads) {
      const uint32_t j = head + gidx * V;
      BinsVec<CT> v;
#pragma unroll
      for (uint32_t i = 0; i < V; ++i) v.v[i] = (CT)tags[j + i];
      *reinterpret_cast<BinsVec<CT> *>(p + j) = v;
    }
    if (tid < ncell - tail0) p[tail0 + tid] = (CT)tags[tail0 + tid];
  } else {
    for (uint32_t j = tid; j < ncell; j += kThreads) {
      const uint32_t row = j / ns, col = j - row * ns;
      out[(row0 + row) * a.ld + c0 + col] = (CT)tags[j];
    }
  }
}

}  // namespace dmlc_amd
