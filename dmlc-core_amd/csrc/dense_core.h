// dense_core.h -- CSR -> dense row batch (dmlc_amd_to_dense): the tile body.
//
// A 256-thread workgroup owns a tile of nr rows x ns columns of `out`
// (dense_shape).  LDS holds one 32-bit tag per cell (0 = no entry) and the
// tile's nr + 1 offsets.
//   A  zero the tags, load the offsets (clamped to the arrays' capacity)
//   B  the threads stride over the tile's contiguous entry range
//      [offset[r0], offset[r0 + nr]) -- per entry, not per row, so one long
//      row among empty ones does not serialise a wave.  Each finds its
//      entry's row in the LDS offsets and does an LDS max of (position in the
//      row) + 1 into the cell: the largest position wins, which is the "last
//      entry wins" of a sequential walk, whatever the scheduling.  Entries
//      with index >= ncol are counted in d_status (global atomics on that
//      path only).
//   C  every cell's owner reads its tag and stores value[offset[row] + tag - 1]
//      or the fill: each element of the window is written exactly once, `out`
//      is never read and never cleared first.  A tile that is one contiguous
//      span of `out` (ld == ncol, no column tiling) stores 16 bytes per lane
//      apart from an unaligned head and tail.
// Values are bit patterns (VT = uint32_t for f32 / i32, uint64_t for i64).
// No workgroup talks to another.  Compiles as HIP device code (block.h) and as
// plain C++ with a host block (tests/emu/dense_check.cpp).
#pragma once
#include "common.h"

namespace dmlc_amd {

constexpr uint32_t kDenseCells = 4096;  // cells per tile (LDS tags)
constexpr uint32_t kDenseRows = 256;    // most rows per tile (LDS offsets)
constexpr uint64_t kDenseMaxTiles = 0x7FFFFFFFull;  // one launch's grid
constexpr uint64_t kDenseMaxRowLen = 0xFFFFFFFFull;  // a row of this many entries does not fit the tag

// d_status words and flag bits (include/dmlc_amd.h)
enum { DS_ROWS = 0, DS_DROPPED = 1, DS_FIRST = 2, DS_FLAGS = 3 };
enum { kDenseFlagError = 1u, kDenseFlagValueCount = 2u, kDenseFlagOffsetCap = 4u, kDenseFlagRowTooLong = 8u };

struct DenseArgs {
  const uint64_t *offset;
  const void *index;
  const void *value;
  const uint64_t *res;  // the parse's device result block (dmlc_amd_result)
  uint64_t cap_rows, cap_index, cap_value;
  uint64_t row_begin, row_end;  // the row window (row_end saturates)
  uint64_t ncol, ld;
  uint64_t fill, one;  // bit patterns of the fill and of DType(1)
  uint32_t S, R;       // columns and rows per tile
  uint32_t col_tiles;
  void *out;
  uint64_t *status;
};

// tile shape for ncol columns
DA_HD void dense_shape(uint64_t ncol, uint32_t *S, uint32_t *R) {
  *S = (uint32_t)mn<uint64_t>(ncol, kDenseCells);
  *R = mn<uint32_t>(kDenseRows, kDenseCells / *S);
}

// flag bits 0 and 1: the parse failed, or its value count fits no RowBlock
// (GetBlock's CHECK, row_block.h:171-189); nothing is written then
DA_HD uint64_t dense_result_flags(const uint64_t *res) {
  uint64_t f = 0;
  if (res[8] != 0) f |= kDenseFlagError;
  if (res[C_VALUE] != 0 && res[C_VALUE] != res[C_INDEX]) f |= kDenseFlagValueCount;
  return f;
}

// one past the last row of the window that exists
DA_HD uint64_t dense_row_end(const DenseArgs &a) {
  return mn<uint64_t>(mn<uint64_t>(a.res[C_ROWS], a.cap_rows), a.row_end);
}

// d_status before the tiles run (one thread)
DA_HD void dense_status_init(const DenseArgs &a) {
  const uint64_t f = dense_result_flags(a.res);
  const uint64_t end = dense_row_end(a);
  a.status[DS_ROWS] = f == 0 && end > a.row_begin ? end - a.row_begin : 0;
  a.status[DS_DROPPED] = 0;
  a.status[DS_FIRST] = kNone;
  a.status[DS_FLAGS] = f;
}

template <typename VT>
struct alignas(16) DenseVec {
  VT v[16 / sizeof(VT)];
};
struct alignas(16) DenseTag4 {
  uint32_t t[4];
};

// tags: kDenseCells words, 16-byte aligned; offs: kDenseRows + 1; bad: one word
template <typename IT, typename VT, class BK>
DA_HDF void dense_tile(const DenseArgs &a, uint64_t tile, uint32_t *tags, uint64_t *offs, uint32_t *bad, BK &bk) {
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

  // ---- A
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
  }
  bk.sync();
  const uint64_t e0 = offs[0], e1 = offs[nr];
  if (e1 - e0 >= kDenseMaxRowLen) {  // (uniform) some row may not fit the tag: look at each
    if (tid == 0) *bad = 0;
    bk.sync();
    for (uint32_t j = tid; j < nr; j += kThreads)
      if (offs[j + 1] - offs[j] >= kDenseMaxRowLen) atomic_or_u32(bad, 1u);
    bk.sync();
    if (*bad != 0) {  // refused: the flag, and nothing of this tile is written
      if (tid == 0) atomic_or_u64(&a.status[DS_FLAGS], kDenseFlagRowTooLong);
      return;
    }
  }

  // ---- B
  if (e1 > e0) {
    const IT *index = static_cast<const IT *>(a.index);
    const float scale = (float)nr / (float)(e1 - e0);
    uint64_t dropped = 0, first = kNone;
    for (uint64_t k = e0 + tid; k < e1; k += kThreads) {
      // the entry's row: the last j with offs[j] <= k (empty rows share an
      // offset with their successor).  Rows of equal length are found by the
      // first guess; otherwise a binary search from it.
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
  bk.sync();

  // ---- C
  const VT *value = static_cast<const VT *>(a.value);
  VT *out = static_cast<VT *>(a.out);
  const VT fill = (VT)a.fill, one = (VT)a.one;
  auto cell = [&](uint32_t row, uint32_t j) -> VT {
    const uint32_t tag = tags[j];
    if (tag == 0) return fill;
    if (!has_val) return one;  // RowBlock::get_value: no value array means 1
    const uint64_t k = offs[row] + tag - 1;
    return k < lim ? value[k] : fill;  // (k < lim always, for ascending offsets)
  };
  const uint64_t row0 = r0 - a.row_begin;
  if (a.ld == a.ncol && a.col_tiles == 1) {
    // one contiguous span of ncell elements
    constexpr uint32_t V = 16 / sizeof(VT);
    VT *p = out + row0 * a.ld;
    const uint32_t mis = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 15u);
    const uint32_t head = mn<uint32_t>(ncell, ((16u - mis) & 15u) / (uint32_t)sizeof(VT));
    const uint32_t ngroup = (ncell - head) / V;
    const uint32_t tail0 = head + ngroup * V;
    if (tid < head) p[tid] = cell(tid / ns, tid);
    for (uint32_t gidx = tid; gidx < ngroup; gidx += kThreads) {
      uint32_t j = head + gidx * V;
      uint32_t row = j / ns, col = j - row * ns;
      DenseVec<VT> v;
#pragma unroll
      for (uint32_t i = 0; i < V; ++i) {
        v.v[i] = cell(row, j + i);
        if (++col == ns) {
          col = 0;
          ++row;
        }
      }
      *reinterpret_cast<DenseVec<VT> *>(p + j) = v;
    }
    if (tid < ncell - tail0) p[tail0 + tid] = cell((tail0 + tid) / ns, tail0 + tid);
  } else {
    for (uint32_t j = tid; j < ncell; j += kThreads) {
      const uint32_t row = j / ns, col = j - row * ns;
      out[(row0 + row) * a.ld + c0 + col] = cell(row, j);
    }
  }
}

}  // namespace dmlc_amd
