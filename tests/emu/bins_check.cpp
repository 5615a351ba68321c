// TEST INFRASTRUCTURE ONLY: the CSR -> bin codes tile body (bins_core.h) on the
// CPU, 256 host threads per tile, for every index type and code width, against
// a sequential loop that restates include/dmlc_amd.h's semantics.  The whole
// output buffer (padding, rows past the window and guard bytes included) and
// the eight status words must be equal.  One line per case; the last line
// carries the totals tests/test_emu_bins.py reads.
// usage: bins_check [seed]
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bins_core.h"

using namespace dmlc_amd;

namespace {

struct Barrier {
  std::mutex m;
  std::condition_variable cv;
  int n, waiting = 0;
  unsigned gen = 0;
  explicit Barrier(int n_) : n(n_) {}
  void wait() {
    std::unique_lock<std::mutex> lk(m);
    const unsigned g = gen;
    if (++waiting == n) {
      waiting = 0;
      ++gen;
      cv.notify_all();
    } else {
      cv.wait(lk, [&] { return gen != g; });
    }
  }
};
struct HostBlk {  // the block policy: thread id and workgroup barrier
  int t;
  Barrier *bar;
  int tid() const { return t; }
  void sync() { bar->wait(); }
};

uint64_t st = 88172645463325252ull;
uint64_t rnd() {
  st ^= st << 13;
  st ^= st >> 7;
  st ^= st << 17;
  return st;
}

const uint32_t kNanPayload = 0x7FC01234u;

// one case, independent of the index type and the code width
struct Case {
  std::string name;
  std::vector<uint64_t> offset, index;
  std::vector<uint32_t> value;  // float bit patterns
  std::vector<uint32_t> cut_ptr;
  std::vector<float> cut_value;  // may hold more than n_cuts
  uint64_t n_cuts = 0;
  uint64_t count[8] = {0, 0, 0, 0, 0, 0, 0, 0}, error = 0;
  uint64_t cap_rows = 0, cap_index = 0;
  uint64_t row_begin = 0, max_rows = 0, ncol = 1, ld = 1;
  uint32_t out_shift = 0;  // out starts this many elements into its buffer
  uint32_t missing = 0xFFFFFFFFu;  // masked to the code width
  bool global_ids = false;
  bool wide_only = false;  // holds indices >= 2^32
  bool unspecified = false;  // some column's cuts are not ascending: only the accesses and status words 0 - 2 are checked
};

// cuts that are not ascending in some columns (a 0.0 now and then), the counts drawn from `menu`
void make_unsorted_cuts(Case &c, const std::vector<uint32_t> &menu) {
  c.cut_ptr.assign(1, 0);
  c.cut_value.clear();
  for (uint64_t col = 0; col < c.ncol; ++col) {
    const uint32_t m = menu[rnd() % menu.size()];
    float x = (float)((int)(rnd() % 200) - 100);
    for (uint32_t i = 0; i < m; ++i) {
      c.cut_value.push_back(rnd() % 16 == 0 ? 0.0f : x);
      x += (float)(rnd() % 4) * 0.25f;
    }
    c.cut_ptr.push_back((uint32_t)c.cut_value.size());
  }
  c.n_cuts = c.cut_value.size();
}

// one ascending table: whatever range of it a column owns is ascending
void ascending_table(Case &c) {
  for (size_t i = 0; i < c.cut_value.size(); ++i) c.cut_value[i] = -20.0f + 0.25f * (float)i;
}

// usable cuts (ascending inside every column): what the semantics define
void make_sorted_cuts(Case &c, const std::vector<uint32_t> &menu) {
  c.cut_ptr.assign(1, 0);
  c.cut_value.clear();
  for (uint64_t col = 0; col < c.ncol; ++col) {
    const uint32_t m = menu[rnd() % menu.size()];
    float x = (float)((int)(rnd() % 200) - 100);
    for (uint32_t i = 0; i < m; ++i) {
      c.cut_value.push_back(x);
      x += (float)(rnd() % 4) * 0.25f;  // equal neighbours occur
    }
    c.cut_ptr.push_back((uint32_t)c.cut_value.size());
  }
  c.n_cuts = c.cut_value.size();
}

uint32_t fbits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

// a value for column col: one of its cuts, a neighbour of one, or a special
uint32_t pick_value(const Case &c, uint64_t col) {
  const uint32_t b = c.cut_ptr[col], e = c.cut_ptr[col + 1];
  const uint64_t r = rnd();
  if (b < e && e <= c.cut_value.size() && r % 4 != 0) {
    const float q = c.cut_value[b + (rnd() % (e - b))];
    switch (r % 3) {
      case 0: return fbits(q);
      case 1: return fbits(std::nextafterf(q, INFINITY));
      default: return fbits(std::nextafterf(q, -INFINITY));
    }
  }
  switch ((r >> 8) % 9) {
    case 0: return 0x00000000u;   // +0
    case 1: return 0x80000000u;   // -0
    case 2: return 0x7F800000u;   // +inf
    case 3: return 0xFF800000u;   // -inf
    case 4: return 0x00000001u;   // the smallest denormal
    case 5: return kNanPayload;   // NaN with a payload
    case 6: return fbits(-1e30f);  // below every cut
    case 7: return fbits(1e30f);   // above every cut
    default: return fbits((float)((int)(rnd() % 400) - 200) * 0.125f);
  }
}

// rows of random entries: about `per_row` entries per row, columns below `cmax`; cuts from `menu`
Case random_case(const std::string &name, uint64_t rows, uint64_t ncol, double per_row, uint64_t cmax, uint64_t extra_ld,
                 const std::vector<uint32_t> &menu, bool values = true) {
  Case c;
  c.name = name;
  c.ncol = ncol;
  make_sorted_cuts(c, menu);
  c.offset.push_back(0);
  for (uint64_t r = 0; r < rows; ++r) {
    const uint64_t m = per_row <= 0 ? 0 : rnd() % (uint64_t)(2 * per_row + 1);
    for (uint64_t i = 0; i < m; ++i) {
      const uint64_t col = rnd() % cmax;
      c.index.push_back(col);
      c.value.push_back(col < ncol ? pick_value(c, col) : 0u);
    }
    c.offset.push_back(c.index.size());
  }
  if (!values) c.value.clear();
  c.count[C_ROWS] = rows;
  c.count[C_INDEX] = c.index.size();
  c.count[C_VALUE] = c.value.size();
  c.cap_rows = rows;
  c.cap_index = c.index.size();
  c.max_rows = rows;
  c.ld = ncol + extra_ld;
  return c;
}

// fresh values for the cuts the case holds now
void redraw_values(Case &c) {
  for (size_t k = 0; k < c.value.size(); ++k)
    if (c.index[k] < c.ncol) c.value[k] = pick_value(c, c.index[k]);
}

struct Job {
  std::string name;
  BinsArgs b;
  int wide, cbytes;
  bool unspecified;
  uint64_t ntiles, row_tiles;
  bool staged = false, staged_groups = false, from_global = false;
  std::vector<uint64_t> offset;
  std::vector<unsigned char> index, out, expect;
  std::vector<uint32_t> value, cut_ptr;
  std::unique_ptr<float[]> cut_value;  // exactly n_cuts floats: a read at or past n_cuts is a heap overflow
  uint64_t res[16];
  uint64_t status[8], want[8];
};

template <typename T>
void put(std::vector<unsigned char> &b, size_t i, T v) {
  std::memcpy(b.data() + i * sizeof(T), &v, sizeof(T));
}

// the sequential statement of the semantics
template <typename IT, typename CT>
void reference(Job &j, const Case &c) {
  for (int i = 0; i < 8; ++i) j.want[i] = 0;
  j.want[2] = ~0ull;
  if (c.error) j.want[3] |= 1;
  if (c.count[C_VALUE] != 0 && c.count[C_VALUE] != c.count[C_INDEX]) j.want[3] |= 2;
  if (j.want[3]) return;
  const bool has_val = c.count[C_VALUE] != 0;
  const uint64_t lim = has_val ? mn<uint64_t>(j.b.d.cap_index, j.b.d.cap_value) : j.b.d.cap_index;
  const uint64_t rows = mn<uint64_t>(c.count[C_ROWS], c.cap_rows);
  const uint64_t end = mn<uint64_t>(rows, c.row_begin + c.max_rows);
  const IT *index = reinterpret_cast<const IT *>(j.index.data());
  CT *out = reinterpret_cast<CT *>(j.expect.data()) + c.out_shift;
  const uint64_t top = sizeof(CT) == 4 ? 0xFFFFFFFFull : (1ull << (8 * sizeof(CT))) - 1;
  std::vector<int64_t> win(c.ncol);
  // a row of 2^32 - 1 or more entries (after the clamp to the capacity): flag bit 3, and the rows of its tile --
  // R rows from row_begin on, whatever the column tile -- are not written, their dropped entries not counted
  const uint64_t R = j.b.d.R;
  auto clamped = [&](uint64_t r) { return mn<uint64_t>(c.offset[r], lim); };
  std::vector<char> refused((end > c.row_begin ? (end - c.row_begin - 1) / R + 1 : 0), 0);
  for (uint64_t r = c.row_begin; r < end; ++r)
    if (clamped(r + 1) - clamped(r) >= kDenseMaxRowLen) {
      refused[(r - c.row_begin) / R] = 1;
      j.want[3] |= kDenseFlagRowTooLong;
    }
  for (uint64_t r = c.row_begin; r < end; ++r) {
    for (uint64_t x = 0; x < c.ncol; ++x) win[x] = -1;
    if (c.offset[r] > lim || c.offset[r + 1] > lim) j.want[3] |= 4;
    ++j.want[0];
    if (refused[(r - c.row_begin) / R]) continue;
    for (uint64_t k = c.offset[r]; k < c.offset[r + 1]; ++k) {
      if (k >= lim) continue;
      const uint64_t col = (uint64_t)index[k];
      if (col < c.ncol) {
        win[col] = (int64_t)k;
      } else {
        ++j.want[1];
        j.want[2] = mn<uint64_t>(j.want[2], k);
      }
    }
    for (uint64_t x = 0; x < c.ncol; ++x) {
      uint64_t code = j.b.missing;
      if (win[x] >= 0) {
        const float v = has_val ? u2f(j.value[(size_t)win[x]]) : 1.0f;
        const uint64_t b = j.cut_ptr[x], e = j.cut_ptr[x + 1];
        if (b > e || e > c.n_cuts) {
          ++j.want[5];
          j.want[3] |= kBinsFlagCutPtr;
        } else if (e == b) {
          ++j.want[5];
        } else if (v != v) {
          ++j.want[4];
        } else {
          uint64_t n = 0;
          for (uint64_t i = b; i < e; ++i) n += j.cut_value[i] <= v;
          uint64_t code2 = mn<uint64_t>(n, e - b - 1) + (c.global_ids ? b : 0);
          if (code2 > top || code2 == j.b.missing) j.want[3] |= kBinsFlagCodeRange;
          else code = code2;
        }
      }
      out[(r - c.row_begin) * c.ld + x] = (CT)code;
    }
  }
}

template <typename IT, typename CT>
Job *make_job(const Case &c) {
  Job *j = new Job;
  j->name = c.name + (sizeof(IT) == 8 ? "/u64" : "/u32") + "/c" + std::to_string(sizeof(CT));
  j->wide = sizeof(IT) == 8;
  j->cbytes = (int)sizeof(CT);
  j->unspecified = c.unspecified;
  j->offset = c.offset;
  // the arrays hold what the case lists, which may be more than the capacity says (a sentinel tail)
  j->index.assign((c.index.size() + 1) * sizeof(IT), 0);
  for (size_t i = 0; i < c.index.size(); ++i) put<IT>(j->index, i, (IT)c.index[i]);
  j->value = c.value;
  j->value.push_back(0);
  j->cut_ptr = c.cut_ptr;
  j->cut_value.reset(new float[c.n_cuts]);
  for (uint64_t i = 0; i < c.n_cuts; ++i) j->cut_value[i] = c.cut_value[i];
  std::memset(j->res, 0, sizeof(j->res));
  for (int i = 0; i < 8; ++i) j->res[i] = c.count[i];
  j->res[8] = c.error;
  const uint64_t rows_out = c.max_rows + 2;  // two guard rows
  j->out.assign((rows_out * c.ld + c.out_shift + 4) * sizeof(CT) + 32, 0xA5);
  j->expect = j->out;
  BinsArgs &b = j->b;
  std::memset(&b, 0, sizeof(b));
  DenseArgs &a = b.d;
  dense_shape(c.ncol, &a.S, &a.R);
  const uint64_t nrows = c.row_begin < c.cap_rows ? mn<uint64_t>(c.max_rows, c.cap_rows - c.row_begin) : 0;
  const uint64_t col_tiles = (c.ncol - 1) / a.S + 1;
  j->row_tiles = nrows ? (nrows - 1) / a.R + 1 : 0;
  j->ntiles = col_tiles * j->row_tiles;
  a.offset = j->offset.data();
  a.index = j->index.data();
  a.value = c.value.empty() ? nullptr : j->value.data();
  a.res = j->res;
  a.cap_rows = c.cap_rows;
  a.cap_index = c.cap_index;
  a.cap_value = c.value.empty() ? 0 : c.cap_index;
  a.row_begin = c.row_begin;
  a.row_end = c.row_begin + c.max_rows;
  a.ncol = c.ncol;
  a.ld = c.ld;
  a.one = 0x3F800000ull;
  a.col_tiles = (uint32_t)col_tiles;
  // the buffers come from operator new: 16-byte aligned, as a device allocation is; then the case's shift
  if ((reinterpret_cast<uintptr_t>(j->out.data()) | reinterpret_cast<uintptr_t>(j->expect.data())) & 15u) {
    std::printf("unaligned test buffer\n");
    std::exit(2);
  }
  a.out = j->out.data() + c.out_shift * sizeof(CT);
  a.status = j->status;
  b.cut_ptr = j->cut_ptr.data();
  b.cut_value = j->cut_value.get();
  b.n_cuts = c.n_cuts;
  b.missing = sizeof(CT) == 4 ? c.missing : c.missing & ((1u << (8 * sizeof(CT))) - 1);
  b.global_ids = c.global_ids;
  reference<IT, CT>(*j, c);
  return j;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  const uint64_t C = kDenseCells, R = kDenseRows;
  const std::vector<uint32_t> kAll = {0, 1, 2, 3, 255, 256, 257}, kSmall = {0, 1, 2, 3}, kMostlySmall = {0, 1, 2, 3, 1, 2, 3, 2, 3, 1, 2, 3, 255, 256, 257};
  std::vector<Case> cases;
  // ---- column counts x row counts (0 rows, 1 row, 1 / 2 / 3 row tiles with a partial last one), both strides,
  // an out starting 1, 3 and 15 elements into its buffer
  for (uint64_t ncol : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)15, (uint64_t)16, (uint64_t)17, (uint64_t)63, (uint64_t)64,
                        (uint64_t)65, C - 1, C, C + 1, 2 * C + 3}) {
    uint32_t S, Rt;
    dense_shape(ncol, &S, &Rt);
    const uint64_t rows_list[5] = {0, 1, Rt > 1 ? (uint64_t)Rt - 1 : 1, (uint64_t)Rt + 1, 2 * (uint64_t)Rt + 1};
    const std::vector<uint32_t> &menu = ncol <= 3 ? kSmall : (ncol <= 65 ? kAll : kMostlySmall);
    for (int ri = 0; ri < 5; ++ri) {
      const uint64_t rows = rows_list[ri];
      const double per_row = ncol < 8 ? 1.5 : (ncol > 1000 ? 40 : 6);
      const std::string nm = "shape/" + std::to_string(ncol) + "x" + std::to_string(rows);
      cases.push_back(random_case(nm + "/ld=ncol", rows, ncol, per_row, ncol, 0, menu));
      cases.push_back(random_case(nm + "/ld+5", rows, ncol, per_row, ncol, 5, menu));
      const uint32_t shift = ri % 3 == 0 ? 1 : (ri % 3 == 1 ? 3 : 15);
      Case s = random_case(nm + "/shift" + std::to_string(shift), rows, ncol, per_row, ncol, 0, menu);
      s.out_shift = shift;
      cases.push_back(s);
    }
  }
  // ---- dense rows (every column once, in order: the CSV shape): 3 cuts a column (staged in LDS, one group) and 256 cuts a column
  // (staged too under bins_core.h's rule, in groups of 16 columns: the only cases that walk several groups; the
  // global-memory path is run by the wide sparse cases).  The totals line counts both, so a change of the rule that
  // drops one shows in tests/test_emu_bins.py
  for (int big = 0; big < 2; ++big)
    for (uint64_t ncol : {(uint64_t)16, (uint64_t)256, (uint64_t)300}) {
      Case c = random_case(std::string("dense/") + (big ? "256cuts/" : "3cuts/") + std::to_string(ncol), 0, ncol, 0, ncol, 0,
                           big ? std::vector<uint32_t>{256} : std::vector<uint32_t>{3});
      const uint64_t rows = 2 * (C / ncol) + 3;
      for (uint64_t r = 0; r < rows; ++r) {
        for (uint64_t x = 0; x < ncol; ++x) {
          c.index.push_back(x);
          c.value.push_back(pick_value(c, x));
        }
        c.offset.push_back(c.index.size());
      }
      c.count[C_ROWS] = c.cap_rows = c.max_rows = rows;
      c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
      c.missing = big ? 0xFFFFFF00u : 0xFFFFFFFFu;  // (256 cuts and missing 255 would flag every top code)
      cases.push_back(c);
    }
  // ---- no value array: every present cell gets the code of 1.0f
  cases.push_back(random_case("novalue/40x700", 700, 40, 5, 40, 0, kAll, false));
  cases.push_back(random_case("novalue/40x700/ld+5", 700, 40, 5, 40, 5, kSmall, false));
  // ---- duplicates: the last entry of a cell wins, a NaN included
  {
    Case c = random_case("dup/near+far+stride", 0, 500, 0, 500, 0, kMostlySmall);
    for (uint64_t i = 0; i < 700; ++i) {
      uint64_t col = i % 500;
      if (i == 10 || i == 20 || i == 33) col = 7;           // one wave's stretch
      if (i == 100 || i == 400) col = 450;                  // 300 apart
      if (i == 5 || i == 261 || i == 517) col = 499;        // the threads' stride
      c.index.push_back(col);
      c.value.push_back(i == 33 ? kNanPayload : pick_value(c, col));
    }
    c.offset.push_back(c.index.size());
    c.count[C_ROWS] = c.cap_rows = c.max_rows = 1;
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
    cases.push_back(c);
  }
  // ---- row skew
  {
    Case c = random_case("skew/5000-in-200", 0, 300, 0, 300, 0, kAll);
    for (int r = 0; r < 201; ++r) {
      if (r == 77)
        for (int i = 0; i < 5000; ++i) {
          const uint64_t col = rnd() % 300;
          c.index.push_back(col);
          c.value.push_back(pick_value(c, col));
        }
      c.offset.push_back(c.index.size());
    }
    c.count[C_ROWS] = c.cap_rows = c.max_rows = 201;
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
    cases.push_back(c);
    cases.push_back(random_case("skew/all-empty", 600, 9, 0, 9, 0, kSmall));
  }
  // ---- row windows: row_begin inside a tile, max_rows short of the end, max_rows past the end
  for (uint64_t extra : {(uint64_t)0, (uint64_t)5}) {
    Case w = random_case("window/begin-inside/" + std::to_string(extra), 3 * R, 20, 5, 20, extra, kAll);
    w.row_begin = 100;
    w.max_rows = 3 * R - 100;
    cases.push_back(w);
    w.name = "window/short/" + std::to_string(extra);
    w.row_begin = 7;
    w.max_rows = 301;
    cases.push_back(w);
    w.name = "window/past-end/" + std::to_string(extra);
    w.row_begin = 3 * R - 250;
    w.max_rows = 400;
    w.cap_rows = 3 * R + 1000;  // upper-bound buffers: the parsed count ends the window
    w.offset.resize(w.cap_rows + 1, 0xDEADull << 40);
    cases.push_back(w);
    w.name = "window/begin-past-rows/" + std::to_string(extra);
    w.row_begin = 3 * R + 10;
    cases.push_back(w);
  }
  // ---- dropped entries: index >= ncol (column-tiled as well: counted once)
  for (uint64_t ncol : {(uint64_t)50, 2 * C + 3}) {
    uint32_t S, Rt;
    dense_shape(ncol, &S, &Rt);
    cases.push_back(random_case("dropped/" + std::to_string(ncol), 2 * (uint64_t)Rt + 1, ncol, ncol > 1000 ? 30 : 8, ncol + ncol / 4, 0,
                                kMostlySmall));
  }
  {
    Case d = random_case("dropped/wide-index", 300, 50, 6, 50, 0, kAll);
    for (size_t i = 0; i < d.index.size(); i += 7) d.index[i] |= 1ull << 32;  // low 32 bits < ncol: dropped, not wrapped
    d.wide_only = true;
    cases.push_back(d);
  }
  // ---- the dense flags
  {
    Case f = random_case("flag/value-count", 50, 20, 5, 20, 0, kAll);
    f.count[C_VALUE] = f.count[C_INDEX] - 1;
    cases.push_back(f);
    Case e = random_case("flag/error", 50, 20, 5, 20, 0, kAll);
    e.error = (123ull << 16) | 3;
    cases.push_back(e);
    // offsets past the index capacity: the arrays' tail past it is a sentinel that must not reach out
    Case o = random_case("flag/offset-cap", 400, 20, 5, 20, 5, kAll);
    o.cap_index = o.offset[250] - 2;
    for (size_t i = o.cap_index; i < o.index.size(); ++i) {
      o.index[i] = 1;
      o.value[i] = fbits(1e30f);
    }
    cases.push_back(o);
  }
  // ---- ROW_TOO_LONG: the last tile holds a row of 2^32 - 1 entries (the rows after it are empty).  The tile
  // leaves before it reads an index or a value, so the arrays hold only the entries before that row;
  // the earlier tiles are written, the refused tile keeps the sentinel.  With
  // ncol > C every row is a tile of its own, in several column tiles.
  for (uint64_t ncol : {(uint64_t)20, C + 9}) {
    uint32_t S, Rt;
    dense_shape(ncol, &S, &Rt);
    const uint64_t rows = 2 * (uint64_t)Rt + (Rt > 1 ? Rt / 2 : 3);
    Case c = random_case("toolong/" + std::to_string(ncol), rows, ncol, ncol > 1000 ? 40 : 5, ncol, ncol > 1000 ? 0 : 5, kMostlySmall);
    const uint64_t at = 2 * (uint64_t)Rt + 1;  // a row of the last tile
    const uint64_t kept = c.offset[at];
    for (uint64_t r = at + 1; r <= rows; ++r) c.offset[r] = kept + 0xFFFFFFFFull;
    c.index.resize(kept);
    c.value.resize(kept);
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = kept + 0xFFFFFFFFull;
    cases.push_back(c);
  }
  // ---- CODE_RANGE: 257 cuts in one byte; 256 cuts with missing_code 255; 255 cuts with missing_code 255 (no flag)
  for (uint32_t m : {257u, 256u, 255u}) {
    Case c = random_case("range/" + std::to_string(m) + "cuts", 40, 6, 4, 6, 0, std::vector<uint32_t>{m});
    for (size_t k = 0; k < c.value.size(); k += 3) c.value[k] = fbits(1e30f);  // the top code
    c.missing = 0xFFFFFFFFu;
    cases.push_back(c);
  }
  {
    // a low missing_code: every cell whose code is 1 takes it and is flagged, at every width
    Case c = random_case("range/missing=1", 300, 17, 6, 17, 5, kAll);
    c.missing = 1;
    cases.push_back(c);
  }
  // ---- CUT_PTR: descending at one column; past n_cuts (the job's array ends there); both column-tiled too
  for (uint64_t ncol : {(uint64_t)12, C + 9}) {
    Case c = random_case("cutptr/descending/" + std::to_string(ncol), 30, ncol, ncol > 1000 ? 60 : 8, ncol, 0, std::vector<uint32_t>{1, 2, 3});
    c.cut_ptr[6] = c.cut_ptr[5] - 1;  // column 5 descends; column 6 starts inside column 4's cuts
    c.index[0] = 5;                   // (and holds an entry)
    ascending_table(c);
    redraw_values(c);
    cases.push_back(c);
    Case p = random_case("cutptr/past-n_cuts/" + std::to_string(ncol), 30, ncol, ncol > 1000 ? 60 : 8, ncol, 5, std::vector<uint32_t>{1, 2, 3});
    p.n_cuts = p.cut_ptr[ncol - 2];  // the last two columns' cuts lie past the capacity
    p.index[0] = ncol - 1;
    cases.push_back(p);
  }
  // ---- the tile's first column descends: the other columns' cuts lie outside [cut_ptr[c0], cut_ptr[c0 + ns]), so
  // the tile cannot stage one range and reads global memory although the cuts are few
  {
    Case c = random_case("scattered/first-descends", 200, 30, 8, 30, 0, std::vector<uint32_t>{4});
    c.cut_ptr[0] = (uint32_t)c.n_cuts;
    cases.push_back(c);
    Case g = random_case("scattered/unsorted-cuts", 200, 30, 8, 30, 0, kSmall);
    make_unsorted_cuts(g, kAll);
    redraw_values(g);
    g.unspecified = true;
    cases.push_back(g);
  }
  // ---- global ids: cut_ptr[c] is added
  {
    Case g = random_case("global/65x300", 300, 65, 6, 65, 0, kAll);
    g.global_ids = true;
    cases.push_back(g);
    Case h = random_case("global/8195x3/ld+5", 3, 2 * C + 3, 40, 2 * C + 3, 5, kMostlySmall);
    h.global_ids = true;
    cases.push_back(h);
  }

  // ---- jobs: every case for every index type and code width
  std::vector<Job *> jobs;
  for (const Case &c : cases) {
    for (int wide = 0; wide < 2; ++wide) {
      if (c.wide_only && !wide) continue;
      if (wide) {
        jobs.push_back(make_job<uint64_t, uint8_t>(c));
        jobs.push_back(make_job<uint64_t, uint16_t>(c));
        jobs.push_back(make_job<uint64_t, uint32_t>(c));
      } else {
        jobs.push_back(make_job<uint32_t, uint8_t>(c));
        jobs.push_back(make_job<uint32_t, uint16_t>(c));
        jobs.push_back(make_job<uint32_t, uint32_t>(c));
      }
    }
  }

  Barrier bar(kThreads);
  alignas(16) static uint32_t tags[kDenseCells];
  static uint64_t offs[kDenseRows + 1];
  static uint32_t cptr[kDenseCells + 1];
  static float lcut[kBinsLdsCuts];
  static uint32_t sm[BL_WORDS];
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      HostBlk bk{t, &bar};
      for (Job *j : jobs) {
        if (t == 0) {
          for (int i = 0; i < 8; ++i) j->status[i] = 0x5555;
          bins_status_init(j->b);
        }
        for (uint64_t tile = 0; tile < j->ntiles; ++tile) {
          if (t == 0) {  // LDS is uninitialised on the GPU
            std::memset(tags, 0xCD, sizeof(tags));
            std::memset(offs, 0xCD, sizeof(offs));
            std::memset(cptr, 0xCD, sizeof(cptr));
            std::memset(lcut, 0xCD, sizeof(lcut));
            std::memset(sm, 0xCD, sizeof(sm));
          }
          bar.wait();
          if (j->wide) {
            if (j->cbytes == 1) bins_tile<uint64_t, uint8_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
            else if (j->cbytes == 2) bins_tile<uint64_t, uint16_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
            else bins_tile<uint64_t, uint32_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
          } else {
            if (j->cbytes == 1) bins_tile<uint32_t, uint8_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
            else if (j->cbytes == 2) bins_tile<uint32_t, uint16_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
            else bins_tile<uint32_t, uint32_t>(j->b, tile, tags, offs, cptr, lcut, sm, bk);
          }
          bar.wait();
          if (t == 0) {  // where this tile's searches read (bins_core.h BL_PATH; untouched by a tile that left early)
            if (sm[BL_PATH] == kBinsPathStaged || sm[BL_PATH] == kBinsPathStagedGroups) j->staged = true;
            if (sm[BL_PATH] == kBinsPathStagedGroups) j->staged_groups = true;
            if (sm[BL_PATH] == kBinsPathGlobal && sm[BL_MMAX] != 0) j->from_global = true;
          }
        }
      }
    });
  for (auto &x : th) x.join();

  long bad = 0;
  uint64_t tiles = 0, coltiled = 0, multirow = 0, dropped = 0, vec = 0, strided = 0, staged = 0, groups = 0, toolong = 0, global = 0, range = 0, cutptr = 0,
           nan = 0, unbinned = 0;
  for (Job *j : jobs) {
    long mism = 0;
    if (!j->unspecified)
      for (size_t i = 0; i < j->out.size(); ++i) mism += j->out[i] != j->expect[i];
    for (int i = 0; i < (j->unspecified ? 3 : 8); ++i) mism += j->status[i] != j->want[i];
    std::printf("%-44s tiles %5llu coltiles %u rowtiles %4llu rows %5llu dropped %6llu flags %llu nan %llu unbinned %llu cuts %s mismatches %ld\n",
                j->name.c_str(), (unsigned long long)j->ntiles, j->b.d.col_tiles, (unsigned long long)j->row_tiles,
                (unsigned long long)j->status[0], (unsigned long long)j->status[1], (unsigned long long)j->status[3],
                (unsigned long long)j->status[4], (unsigned long long)j->status[5],
                j->staged ? (j->from_global ? "lds+global" : "lds") : (j->from_global ? "global" : "none"), mism);
    bad += mism;
    tiles += j->ntiles;
    const bool ran = j->status[0] != 0;
    if (ran && j->b.d.col_tiles > 1) ++coltiled;
    if (ran && j->row_tiles > 1) ++multirow;
    if (j->status[1]) ++dropped;
    if (ran && j->b.d.col_tiles == 1 && j->b.d.ld == j->b.d.ncol) ++vec;
    else if (ran) ++strided;
    if (ran && j->staged) ++staged;
    if (ran && j->staged_groups) ++groups;
    if (j->status[3] & kDenseFlagRowTooLong) ++toolong;
    if (ran && j->from_global) ++global;
    if (j->status[3] & kBinsFlagCodeRange) ++range;
    if (j->status[3] & kBinsFlagCutPtr) ++cutptr;
    if (j->status[4]) ++nan;
    if (j->status[5]) ++unbinned;
    delete j;
  }
  std::printf("cases %zu, jobs %zu, tiles %llu, column-tiled %llu, multi-row-tile %llu, dropped %llu, contiguous %llu, strided %llu, "
              "lds-cuts %llu, lds-groups %llu, global-cuts %llu, row-too-long %llu, code-range %llu, cut-ptr %llu, nan %llu, unbinned %llu, mismatches %ld\n",
              cases.size(), jobs.size(), (unsigned long long)tiles, (unsigned long long)coltiled, (unsigned long long)multirow,
              (unsigned long long)dropped, (unsigned long long)vec, (unsigned long long)strided, (unsigned long long)staged,
              (unsigned long long)groups, (unsigned long long)global, (unsigned long long)toolong, (unsigned long long)range, (unsigned long long)cutptr, (unsigned long long)nan,
              (unsigned long long)unbinned, bad);
  return bad != 0;
}
