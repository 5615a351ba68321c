// TEST INFRASTRUCTURE ONLY: the CSR -> dense tile body (dense_core.h) on the
// CPU, 256 host threads per tile, for every index / value type, against a
// sequential loop that restates include/dmlc_amd.h's semantics.  The whole
// output buffer (padding, rows past the window and guard words included) and
// the four status words must be equal.  One line per case; the last line
// carries the totals tests/test_emu_dense.py reads.
// usage: dense_check [seed]
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "dense_core.h"

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

// one case, independent of the index / value types
struct Case {
  std::string name;
  std::vector<uint64_t> offset, index, value;  // value: bit patterns
  uint64_t count[8] = {0, 0, 0, 0, 0, 0, 0, 0}, error = 0;
  uint64_t cap_rows = 0, cap_index = 0;  // capacities (the arrays hold at least as much)
  uint64_t row_begin = 0, max_rows = 0, ncol = 1, ld = 1, fill = 0;
  uint32_t out_shift = 0;  // out starts this many elements into its buffer
  bool wide_only = false;  // holds indices >= 2^32
};

const uint64_t kSentinel = 0xA5A5A5A5A5A5A5A5ull;

// rows of random entries: about `per_row` entries per row, columns below `cmax`
Case random_case(const std::string &name, uint64_t rows, uint64_t ncol, double per_row, uint64_t cmax, uint64_t extra_ld,
                 bool values = true) {
  Case c;
  c.name = name;
  c.offset.push_back(0);
  for (uint64_t r = 0; r < rows; ++r) {
    const uint64_t m = per_row <= 0 ? 0 : rnd() % (uint64_t)(2 * per_row + 1);
    for (uint64_t i = 0; i < m; ++i) {
      c.index.push_back(rnd() % cmax);
      c.value.push_back(rnd() | 1);
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
  c.ncol = ncol;
  c.ld = ncol + extra_ld;
  c.fill = 0x7FC0123400000000ull | 0x7FC01234ull;
  return c;
}

struct Job {
  std::string name;
  DenseArgs a;
  int wide, vbytes;
  uint64_t ntiles, row_tiles;
  std::vector<uint64_t> offset;
  std::vector<unsigned char> index, value, out, expect;
  uint64_t res[16];
  uint64_t status[4], want[4];
};

template <typename T>
void put(std::vector<unsigned char> &b, size_t i, T v) {
  std::memcpy(b.data() + i * sizeof(T), &v, sizeof(T));
}

// the sequential statement of the semantics
template <typename IT, typename VT>
void reference(Job &j, const Case &c) {
  j.want[0] = j.want[1] = j.want[3] = 0;
  j.want[2] = ~0ull;
  if (c.error) j.want[3] |= 1;
  if (c.count[C_VALUE] != 0 && c.count[C_VALUE] != c.count[C_INDEX]) j.want[3] |= 2;
  if (j.want[3]) return;
  const bool has_val = c.count[C_VALUE] != 0;
  const uint64_t lim = has_val ? mn<uint64_t>(j.a.cap_index, j.a.cap_value) : j.a.cap_index;
  const uint64_t rows = mn<uint64_t>(c.count[C_ROWS], c.cap_rows);
  const uint64_t end = mn<uint64_t>(rows, c.row_begin + c.max_rows);
  const IT *index = reinterpret_cast<const IT *>(j.index.data());
  const VT *value = reinterpret_cast<const VT *>(j.value.data());
  VT *out = reinterpret_cast<VT *>(j.expect.data()) + c.out_shift;
  for (uint64_t r = c.row_begin; r < end; ++r) {
    for (uint64_t x = 0; x < c.ncol; ++x) out[(r - c.row_begin) * c.ld + x] = (VT)c.fill;
    if (c.offset[r] > lim || c.offset[r + 1] > lim) j.want[3] |= 4;
    for (uint64_t k = c.offset[r]; k < c.offset[r + 1]; ++k) {
      if (k >= lim) continue;
      const uint64_t col = (uint64_t)index[k];
      if (col < c.ncol) {
        out[(r - c.row_begin) * c.ld + col] = has_val ? value[k] : (VT)j.a.one;
      } else {
        ++j.want[1];
        j.want[2] = mn<uint64_t>(j.want[2], k);
      }
    }
    ++j.want[0];
  }
}

template <typename IT, typename VT>
Job *make_job(const Case &c, int vtype) {
  Job *j = new Job;
  j->name = c.name + (sizeof(IT) == 8 ? "/u64" : "/u32") + (vtype == 0 ? "/f32" : vtype == 1 ? "/i32" : "/i64");
  j->wide = sizeof(IT) == 8;
  j->vbytes = (int)sizeof(VT);
  j->offset = c.offset;
  // the arrays hold what the case lists, which may be more than the capacity says (a sentinel tail)
  j->index.assign((c.index.size() + 1) * sizeof(IT), 0);
  for (size_t i = 0; i < c.index.size(); ++i) put<IT>(j->index, i, (IT)c.index[i]);
  j->value.assign((c.value.size() + 1) * sizeof(VT), 0);
  for (size_t i = 0; i < c.value.size(); ++i) put<VT>(j->value, i, (VT)c.value[i]);
  std::memset(j->res, 0, sizeof(j->res));
  for (int i = 0; i < 8; ++i) j->res[i] = c.count[i];
  j->res[8] = c.error;
  const uint64_t rows_out = c.max_rows + 2;  // two guard rows
  j->out.assign((rows_out * c.ld + c.out_shift + 4) * sizeof(VT) + 16, 0);
  for (size_t i = 0; i + 8 <= j->out.size(); i += 8) std::memcpy(j->out.data() + i, &kSentinel, 8);
  j->expect = j->out;
  DenseArgs &a = j->a;
  std::memset(&a, 0, sizeof(a));
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
  a.fill = sizeof(VT) == 8 ? c.fill : (c.fill & 0xFFFFFFFFull);
  a.one = vtype == 0 ? 0x3F800000ull : 1ull;
  a.col_tiles = (uint32_t)col_tiles;
  // the buffers come from operator new: 16-byte aligned, as a device allocation is; then the case's shift
  if ((reinterpret_cast<uintptr_t>(j->out.data()) | reinterpret_cast<uintptr_t>(j->expect.data())) & 15u) {
    std::printf("unaligned test buffer\n");
    std::exit(2);
  }
  a.out = j->out.data() + c.out_shift * sizeof(VT);
  a.status = j->status;
  reference<IT, VT>(*j, c);
  return j;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  const uint64_t C = kDenseCells, R = kDenseRows;
  std::vector<Case> cases;
  // ---- column counts x row counts (0 rows, 1 row, 1 / 2 / 3 row tiles with a partial last one), both strides,
  // an out starting one element into its buffer
  for (uint64_t ncol : {(uint64_t)1, (uint64_t)2, (uint64_t)3, (uint64_t)63, (uint64_t)64, (uint64_t)65, C - 1, C, C + 1, 2 * C + 3}) {
    uint32_t S, Rt;
    dense_shape(ncol, &S, &Rt);
    const uint64_t rows_list[5] = {0, 1, Rt > 1 ? (uint64_t)Rt - 1 : 1, (uint64_t)Rt + 1, 2 * (uint64_t)Rt + 1};
    for (int ri = 0; ri < 5; ++ri) {
      const uint64_t rows = rows_list[ri];
      const double per_row = ncol < 8 ? 1.5 : (ncol > 1000 ? 40 : 6);
      const std::string nm = "shape/" + std::to_string(ncol) + "x" + std::to_string(rows);
      cases.push_back(random_case(nm + "/ld=ncol", rows, ncol, per_row, ncol, 0));
      Case p = random_case(nm + "/ld+5", rows, ncol, per_row, ncol, 5);
      cases.push_back(p);
      Case s = random_case(nm + "/shift1", rows, ncol, per_row, ncol, 0);
      s.out_shift = 1;
      cases.push_back(s);
    }
  }
  // ---- dense rows (every column once, in order: the CSV shape) and values absent
  for (uint64_t ncol : {(uint64_t)16, (uint64_t)256, (uint64_t)300}) {
    Case c = random_case("dense/" + std::to_string(ncol), 0, ncol, 0, ncol, 0);
    const uint64_t rows = 2 * (C / ncol) + 3;
    for (uint64_t r = 0; r < rows; ++r) {
      for (uint64_t x = 0; x < ncol; ++x) {
        c.index.push_back(x);
        c.value.push_back(rnd());
      }
      c.offset.push_back(c.index.size());
    }
    c.count[C_ROWS] = c.cap_rows = c.max_rows = rows;
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
    cases.push_back(c);
  }
  cases.push_back(random_case("novalue/40x700", 700, 40, 5, 40, 0, false));
  cases.push_back(random_case("novalue/40x700/ld+5", 700, 40, 5, 40, 5, false));
  // ---- duplicates: inside one 64-entry stretch, 300 entries apart in one row, across a 256-entry stride
  {
    Case c = random_case("dup/near+far+stride", 0, 500, 0, 500, 0);
    for (uint64_t i = 0; i < 700; ++i) {
      uint64_t col = i % 500;
      if (i == 10 || i == 20 || i == 33) col = 7;           // one wave's stretch
      if (i == 100 || i == 400) col = 450;                  // 300 apart
      if (i == 5 || i == 261 || i == 517) col = 499;        // the threads' stride
      c.index.push_back(col);
      c.value.push_back(1000 + i);
    }
    c.offset.push_back(c.index.size());
    c.index.push_back(3);
    c.value.push_back(1);
    c.index.push_back(3);
    c.value.push_back(2);
    c.index.push_back(3);
    c.value.push_back(5);  // "1 3:1 3:2 3:5": cell 3 is 5
    c.offset.push_back(c.index.size());
    c.count[C_ROWS] = c.cap_rows = c.max_rows = 2;
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
    cases.push_back(c);
  }
  // ---- row skew: one 5000-entry row among 200 empty rows; empty first and last rows; all rows empty
  {
    Case c = random_case("skew/5000-in-200", 0, 300, 0, 300, 0);
    for (int r = 0; r < 201; ++r) {
      if (r == 77)
        for (int i = 0; i < 5000; ++i) {
          c.index.push_back(rnd() % 300);
          c.value.push_back(rnd());
        }
      c.offset.push_back(c.index.size());
    }
    c.count[C_ROWS] = c.cap_rows = c.max_rows = 201;
    c.count[C_INDEX] = c.count[C_VALUE] = c.cap_index = c.index.size();
    cases.push_back(c);
    Case e = random_case("skew/empty-ends", 40, 30, 4, 30, 5);
    e.offset[1] = 0;
    e.offset[39] = e.offset[40];
    cases.push_back(e);
    cases.push_back(random_case("skew/all-empty", 600, 9, 0, 9, 0));
    cases.push_back(random_case("skew/all-empty/ld+5", 600, 9, 0, 9, 5));
  }
  // ---- row windows: row_begin inside a tile, max_rows short of the end, max_rows past the end
  for (uint64_t extra : {(uint64_t)0, (uint64_t)5}) {
    Case w = random_case("window/begin-inside/" + std::to_string(extra), 3 * R, 20, 5, 20, extra);  // 204 rows per tile
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
    cases.push_back(random_case("dropped/" + std::to_string(ncol), 2 * (uint64_t)Rt + 1, ncol, ncol > 1000 ? 30 : 8, ncol + ncol / 4, 0));
  }
  {
    Case d = random_case("dropped/wide-index", 300, 50, 6, 50, 0);
    for (size_t i = 0; i < d.index.size(); i += 7) d.index[i] |= 1ull << 32;  // low 32 bits < ncol: dropped, not wrapped
    d.wide_only = true;
    cases.push_back(d);
  }
  // ---- flags
  {
    Case f = random_case("flag/value-count", 50, 20, 5, 20, 0);
    f.count[C_VALUE] = f.count[C_INDEX] - 1;
    cases.push_back(f);
    Case e = random_case("flag/error", 50, 20, 5, 20, 0);
    e.error = (123ull << 16) | 3;
    cases.push_back(e);
    // offsets past the index capacity: the arrays' tail past it is a sentinel that must not reach out
    Case o = random_case("flag/offset-cap", 400, 20, 5, 20, 5);
    o.cap_index = o.offset[250] - 2;
    for (size_t i = o.cap_index; i < o.index.size(); ++i) {
      o.index[i] = 1;
      o.value[i] = 0xBADBADBADBADull;
    }
    cases.push_back(o);
  }

  // ---- jobs: every case for every index and value type
  std::vector<Job *> jobs;
  for (const Case &c : cases) {
    for (int wide = 0; wide < 2; ++wide) {
      if (c.wide_only && !wide) continue;
      for (int vt = 0; vt < 3; ++vt) {
        if (wide) jobs.push_back(vt == 2 ? make_job<uint64_t, uint64_t>(c, vt) : make_job<uint64_t, uint32_t>(c, vt));
        else jobs.push_back(vt == 2 ? make_job<uint32_t, uint64_t>(c, vt) : make_job<uint32_t, uint32_t>(c, vt));
      }
    }
  }

  Barrier bar(kThreads);
  alignas(16) static uint32_t tags[kDenseCells];
  static uint64_t offs[kDenseRows + 1];
  static uint32_t bad_word;
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      HostBlk bk{t, &bar};
      for (Job *j : jobs) {
        if (t == 0) dense_status_init(j->a);
        for (uint64_t tile = 0; tile < j->ntiles; ++tile) {
          if (t == 0) {  // LDS is uninitialised on the GPU
            std::memset(tags, 0xCD, sizeof(tags));
            std::memset(offs, 0xCD, sizeof(offs));
            bad_word = 0xCDCDCDCDu;
          }
          bar.wait();
          if (j->wide) {
            if (j->vbytes == 8) dense_tile<uint64_t, uint64_t>(j->a, tile, tags, offs, &bad_word, bk);
            else dense_tile<uint64_t, uint32_t>(j->a, tile, tags, offs, &bad_word, bk);
          } else {
            if (j->vbytes == 8) dense_tile<uint32_t, uint64_t>(j->a, tile, tags, offs, &bad_word, bk);
            else dense_tile<uint32_t, uint32_t>(j->a, tile, tags, offs, &bad_word, bk);
          }
          bar.wait();
        }
      }
    });
  for (auto &x : th) x.join();

  long bad = 0;
  uint64_t tiles = 0, coltiled = 0, multirow = 0, dropped = 0, vec = 0, strided = 0;
  for (Job *j : jobs) {
    long mism = 0;
    for (size_t i = 0; i < j->out.size(); ++i) mism += j->out[i] != j->expect[i];
    for (int i = 0; i < 4; ++i) mism += j->status[i] != j->want[i];
    std::printf("%-44s tiles %5llu coltiles %u rowtiles %4llu rows %5llu dropped %6llu flags %llu mismatches %ld\n", j->name.c_str(),
                (unsigned long long)j->ntiles, j->a.col_tiles, (unsigned long long)j->row_tiles,
                (unsigned long long)j->status[0], (unsigned long long)j->status[1], (unsigned long long)j->status[3], mism);
    bad += mism;
    tiles += j->ntiles;
    if (j->status[0] && j->a.col_tiles > 1) ++coltiled;
    if (j->status[0] && j->row_tiles > 1) ++multirow;
    if (j->status[1]) ++dropped;
    if (j->status[0] && j->a.col_tiles == 1 && j->a.ld == j->a.ncol) ++vec;
    else if (j->status[0]) ++strided;
    delete j;
  }
  std::printf("cases %zu, jobs %zu, tiles %llu, column-tiled %llu, multi-row-tile %llu, dropped %llu, contiguous %llu, strided %llu, mismatches %ld\n",
              cases.size(), jobs.size(), (unsigned long long)tiles, (unsigned long long)coltiled,
              (unsigned long long)multirow, (unsigned long long)dropped, (unsigned long long)vec,
              (unsigned long long)strided, bad);
  return bad != 0;
}
