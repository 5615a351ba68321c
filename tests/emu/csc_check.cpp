// TEST INFRASTRUCTURE ONLY: the CSC transpose's tile bodies (csc_core.h) on the
// CPU, 256 host threads per tile, for every index / value width, against a
// sequential loop that restates include/dmlc_amd.h's walk.  Every output
// buffer whole (guard words past the capacity and arrays that must stay
// unwritten included) and the four status words must be equal.  One line per
// job; the last line carries the totals tests/test_emu_csc.py reads.
// usage: csc_check [seed]
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "csc_core.h"

using namespace dmlc_amd;

namespace {

// (a spinning barrier that yields: 256 threads on a few cores meet far sooner
// than through a condition variable, and the scatter meets often)
struct Barrier {
  std::atomic<int> waiting{0};
  std::atomic<unsigned> gen{0};
  int n;
  explicit Barrier(int n_) : n(n_) {}
  void wait() {
    const unsigned g = gen.load(std::memory_order_acquire);
    if (waiting.fetch_add(1, std::memory_order_acq_rel) + 1 == n) {
      waiting.store(0, std::memory_order_relaxed);
      gen.store(g + 1, std::memory_order_release);
    } else {
      while (gen.load(std::memory_order_acquire) == g) std::this_thread::yield();
    }
  }
};
// the block policy: thread id, workgroup barrier, exclusive scan, and the
// wave-level ballot and ordering point of DevBlockT (a barrier over the wave's
// 64 threads: every lane of a wave calls them together)
struct HostBlk {
  int t;
  Barrier *bar;
  Barrier *wbar;          // kWaves barriers of kWave threads
  unsigned char *scan;    // kThreads slots of 64 bytes
  unsigned char *votes;   // kThreads
  int tid() const { return t; }
  void sync() { bar->wait(); }
  void wave_sync() { wbar[t / kWave].wait(); }
  uint64_t ballot(bool p) {
    votes[t] = p;
    wave_sync();
    uint64_t m = 0;
    const int w0 = t / kWave * kWave;
    for (int i = 0; i < kWave; ++i) m |= (uint64_t)votes[w0 + i] << i;
    wave_sync();
    return m;
  }
  template <typename T, typename Op>
  T exclusive(T v, T identity, Op op, T *total) {
    static_assert(sizeof(T) <= 64, "scan element");
    std::memcpy(scan + 64 * t, &v, sizeof(T));
    sync();
    T acc = identity, all = identity;
    for (int i = 0; i < kThreads; ++i) {
      T x;
      std::memcpy(&x, scan + 64 * i, sizeof(T));
      if (i < t) acc = op(acc, x);
      all = op(all, x);
    }
    *total = all;
    sync();
    return acc;
  }
};

uint64_t st = 88172645463325252ull;
uint64_t rnd() {
  st ^= st << 13;
  st ^= st >> 7;
  st ^= st << 17;
  return st;
}

// one case, independent of the widths: index / value as 64-bit patterns
struct Case {
  std::string name;
  std::vector<uint64_t> offset, index, value;
  uint64_t res[16] = {0};
  uint64_t cap_rows = 0, cap_index = 0, cap_value = 0;
  uint64_t row_begin = 0, max_rows = ~0ull, ncol = 1, max_entries = 0;
  uint64_t out_cap = 0;
  bool want_val = true, want_pos = true;
  bool wide_only = false;  // holds indices >= 2^32
  bool one_width = false;  // a large case: u32/v4 and u64/v8 only
  bool single = false;     // 258 tiles, or 2^24 col_offset words: u32/v4 only
};

// rows of lo .. hi entries with columns below `colmax`
Case make_case(const std::string &name, uint64_t rows, uint64_t lo, uint64_t hi, uint64_t ncol, uint64_t colmax,
               bool value = true) {
  Case c;
  c.name = name;
  c.ncol = ncol;
  c.offset.push_back(0);
  for (uint64_t r = 0; r < rows; ++r) {
    const uint64_t m = lo + (hi > lo ? rnd() % (hi - lo + 1) : 0);
    for (uint64_t i = 0; i < m; ++i) {
      c.index.push_back(rnd() % colmax);
      if (value) c.value.push_back(rnd() | 1);
    }
    c.offset.push_back(c.index.size());
  }
  return c;
}
// counts, capacities and an output capacity that hold the case exactly
void fit(Case &c) {
  const uint64_t rows = c.offset.size() - 1, nnz = c.index.size();
  c.res[C_ROWS] = rows;
  c.res[C_INDEX] = nnz;
  c.res[C_VALUE] = c.value.empty() ? 0 : nnz;
  c.cap_rows = rows;
  c.cap_index = nnz;
  c.cap_value = c.value.empty() ? 0 : nnz;
  c.out_cap = nnz;
}

struct Job {
  std::string name;
  CscArgs a;
  int wide, vbytes;
  std::vector<unsigned char> index, value, oval, wval;
  std::vector<uint64_t> offset, co, wco, opos, wpos, meta, rec;
  std::vector<uint32_t> orow, wrow, total, hist, bcol[2], brow[2], brpos[2];
  std::vector<unsigned char> bval[2];
  uint64_t res[16], status[4], wstatus[4];
};
const uint64_t kSentinel = 0xA5A5A5A5A5A5A5A5ull;

// the sequential statement of the semantics, on j.w*
void reference(Job &j, const Case &c) {
  uint64_t *ws = j.wstatus;
  ws[0] = ws[1] = ws[3] = 0;
  ws[2] = ~0ull;
  if (c.res[8]) ws[3] |= 1;
  if (c.res[C_VALUE] && c.res[C_VALUE] != c.res[C_INDEX]) ws[3] |= 2;
  if (ws[3]) {
    for (uint64_t k = 0; k <= c.ncol; ++k) j.wco[k] = 0;
    return;
  }
  const bool has_val = c.res[C_VALUE] != 0;
  const uint64_t lim = has_val ? mn<uint64_t>(c.cap_index, c.cap_value) : c.cap_index;
  const uint64_t rows = mn<uint64_t>(c.res[C_ROWS], c.cap_rows);
  const uint64_t r1 = mn<uint64_t>(rows, c.row_begin + c.max_rows < c.row_begin ? ~0ull : c.row_begin + c.max_rows);
  const uint64_t m = c.max_entries ? mn<uint64_t>(c.max_entries, c.cap_index) : c.cap_index;
  struct Ent {
    uint64_t col, row, k;
  };
  std::vector<Ent> ents;
  uint64_t walked = 0;
  for (uint64_t r = c.row_begin; r < r1; ++r) {
    uint64_t o0 = c.offset[r], o1 = c.offset[r + 1];
    if (o0 > lim || o1 > lim) ws[3] |= 4;
    o0 = mn<uint64_t>(o0, lim);
    o1 = mn<uint64_t>(o1, lim);
    for (uint64_t k = o0; k < o1; ++k) {
      if (walked++ >= m) {
        ws[3] |= 16;
        continue;
      }
      const uint64_t col = j.wide ? c.index[k] : (c.index[k] & 0xFFFFFFFFull);
      if (col >= c.ncol) {
        ++ws[1];
        ws[2] = mn<uint64_t>(ws[2], k);
      } else {
        ents.push_back({col, r - c.row_begin, k});
      }
    }
  }
  ws[0] = ents.size();
  if (ents.size() > c.out_cap) ws[3] |= 8;
  // columns in turn, each in walk order
  std::vector<uint64_t> count(c.ncol + 1, 0);
  for (const Ent &e : ents) ++count[e.col + 1];
  for (uint64_t k = 1; k <= c.ncol; ++k) count[k] += count[k - 1];
  for (uint64_t k = 0; k <= c.ncol; ++k) j.wco[k] = count[k];
  for (const Ent &e : ents) {
    const uint64_t d = count[e.col]++;
    if (d >= c.out_cap) continue;
    j.wrow[d] = (uint32_t)e.row;
    if (has_val && c.want_val) std::memcpy(j.wval.data() + d * j.vbytes, &c.value[e.k], j.vbytes);
    if (c.want_pos) j.wpos[d] = e.k;
  }
}

Job *make_job(const Case &c, int wide, int vbytes) {
  Job *j = new Job;
  j->name = c.name + (wide ? "/u64" : "/u32") + (vbytes == 8 ? "/v8" : "/v4");
  j->wide = wide;
  j->vbytes = vbytes;
  const size_t ib = wide ? 8 : 4;
  // the source holds what the case lists (it may be more than the capacity says), and a guard element
  j->index.assign((c.index.size() + 1) * ib, 0xEE);
  for (size_t i = 0; i < c.index.size(); ++i) std::memcpy(j->index.data() + i * ib, &c.index[i], ib);
  j->value.assign((c.value.size() + 1) * vbytes, 0xEE);
  for (size_t i = 0; i < c.value.size(); ++i) std::memcpy(j->value.data() + i * vbytes, &c.value[i], vbytes);
  j->offset = c.offset;
  std::memcpy(j->res, c.res, sizeof(j->res));
  // the outputs: their capacity and two guard elements, all sentinel
  j->co.assign(c.ncol + 3, kSentinel);
  j->orow.assign(c.out_cap + 2, 0xA5A5A5A5u);
  j->oval.assign((c.out_cap + 2) * vbytes, 0xA5);
  j->opos.assign(c.out_cap + 2, kSentinel);
  j->wco = j->co;
  j->wrow = j->orow;
  j->wval = j->oval;
  j->wpos = j->opos;
  CscArgs &a = j->a;
  std::memset(&a, 0, sizeof(a));
  a.offset = j->offset.data();
  a.index = j->index.data();
  a.value = c.value.empty() ? nullptr : j->value.data();
  a.res = j->res;
  a.cap_rows = c.cap_rows;
  a.cap_index = c.cap_index;
  a.cap_value = c.value.empty() ? 0 : c.cap_value;
  a.row_begin = c.row_begin;
  a.row_end = c.row_begin + c.max_rows < c.row_begin ? ~0ull : c.row_begin + c.max_rows;
  a.ncol = c.ncol;
  const uint64_t m = c.max_entries ? mn<uint64_t>(c.max_entries, c.cap_index) : c.cap_index;
  a.max_entries = m;
  a.ntiles = mx<uint64_t>(1, (m + kCscTile - 1) / kCscTile);
  a.passes = csc_passes(c.ncol);
  a.col_offset = j->co.data();
  a.row = j->orow.data();
  a.val = c.want_val ? j->oval.data() : nullptr;
  a.pos = c.want_pos ? j->opos.data() : nullptr;
  a.cap = c.out_cap;
  a.status = j->status;
  // the workspace, every word 0xCD
  j->meta.assign(1, 0xCDCDCDCDCDCDCDCDull);
  j->total.assign(kCscDigits, 0xCDCDCDCDu);
  j->rec.assign(a.ntiles * kCscRecWords, 0xCDCDCDCDCDCDCDCDull);
  j->hist.assign(a.ntiles * kCscDigits, 0xCDCDCDCDu);
  a.meta = j->meta.data();
  a.total = j->total.data();
  a.rec = j->rec.data();
  a.hist = j->hist.data();
  if (a.passes > 1)
    for (int b = 0; b < 2; ++b) {
      j->bcol[b].assign(m + 1, 0xCDCDCDCDu);
      a.buf[b].col = j->bcol[b].data();
      if (b == 1 && a.passes == 2) continue;  // as capi.cpp: the second buffer holds only columns then
      j->brow[b].assign(m + 1, 0xCDCDCDCDu);
      j->brpos[b].assign(m + 1, 0xCDCDCDCDu);
      j->bval[b].assign((m + 1) * vbytes, 0xCD);
      a.buf[b].row = j->brow[b].data();
      a.buf[b].rpos = j->brpos[b].data();
      a.buf[b].val = j->bval[b].data();
    }
  for (int k = 0; k < 4; ++k) j->status[k] = kSentinel;
  reference(*j, c);
  return j;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  const uint64_t T = kCscTile;
  std::vector<Case> cases;
  // ---- entry counts around the tile size, rows of 0 .. 9 entries, one pass
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, T - 1, T, T + 1, 2 * T + 1}) {
    Case c = make_case("count/" + std::to_string(n), 0, 0, 0, 200, 200);
    while (c.index.size() < n) {
      const uint64_t m = mn<uint64_t>(rnd() % 10, n - c.index.size());
      for (uint64_t i = 0; i < m; ++i) {
        c.index.push_back(rnd() % 210);  // some at or past ncol
        c.value.push_back(rnd() | 1);
      }
      c.offset.push_back(c.index.size());
    }
    if (n == 0) c.offset.assign(4, 0);
    fit(c);
    cases.push_back(c);
  }
  // ---- 257 T + 3 entries: the scan's per-thread run is 2 tiles
  {
    Case c = make_case("scanrun/257T+3", 0, 0, 0, 256, 256);
    const uint64_t n = 257 * T + 3;
    c.index.resize(n);
    c.value.resize(n);
    for (uint64_t i = 0; i < n; ++i) {
      c.index[i] = rnd() % 256;
      c.value[i] = i + 1;
      if (i % 37 == 36) c.offset.push_back(i + 1);
    }
    c.offset.push_back(n);
    fit(c);
    c.single = true;
    cases.push_back(c);
  }
  // ---- ncol and the pass count
  for (uint64_t ncol : {1ull, 2ull, 255ull, 256ull, 257ull, 65536ull, 65537ull, 1ull << 24, (1ull << 24) + 1}) {
    Case c = make_case("ncol/" + std::to_string(ncol), 300, 0, 8, ncol, ncol + (ncol > 2 ? 3 : 1));
    if (ncol > 300) {  // the top columns are there
      c.index[0] = ncol - 1;
      c.index[1] = ncol - 2;
      c.index[2] = 0;
    }
    fit(c);
    if (ncol > 70000) c.single = true;
    cases.push_back(c);
  }
  // ---- stability
  {
    Case a = make_case("stable/one-column-ncol1", 700, 0, 2 * (2 * T + 1) / 700, 1, 1);
    fit(a);
    cases.push_back(a);
    Case b = make_case("stable/column-300-of-65537", 40, 0, 2 * (2 * T + 1) / 40, 65537, 1);
    for (auto &x : b.index) x = 300;
    fit(b);
    b.one_width = true;
    cases.push_back(b);
    Case h = make_case("stable/high-digits", 500, 0, 6, 70000, 1);
    for (auto &x : h.index) x = 5 + (rnd() % 3 == 0 ? 0 : rnd() % 2 ? 256 : 65536);
    fit(h);
    cases.push_back(h);
    Case d = make_case("stable/descending-rows", 0, 0, 0, 300, 300);
    for (int r = 0; r < 200; ++r) {
      const int m = (int)(rnd() % 12);
      for (int i = 0; i < m; ++i) {
        d.index.push_back(299 - 3 * i - r % 3);
        d.value.push_back(rnd());
      }
      d.offset.push_back(d.index.size());
    }
    fit(d);
    cases.push_back(d);
    Case t = make_case("stable/same-cell-thrice", 0, 0, 0, 50, 50);
    for (int r = 0; r < 300; ++r) {
      const uint64_t col = rnd() % 50;
      for (int i = 0; i < 3; ++i) {
        t.index.push_back(col);
        t.value.push_back(rnd());
      }
      t.index.push_back(rnd() % 50);
      t.value.push_back(rnd());
      t.offset.push_back(t.index.size());
    }
    fit(t);
    cases.push_back(t);
  }
  // ---- dropped entries
  {
    Case c = make_case("drop/ncol,ncol+1,2^32-1", 400, 1, 6, 100, 100);
    c.index[7] = 100;
    c.index[3] = 101;
    c.index[500] = 0xFFFFFFFFull;
    fit(c);
    cases.push_back(c);
    Case w = c;
    w.name = "drop/2^32+c";
    w.index[2] = (1ull << 32) + 5;
    w.index[600] = (1ull << 32) + 99;
    w.wide_only = true;
    cases.push_back(w);
    Case all = make_case("drop/all", 100, 1, 6, 10, 10);
    for (auto &x : all.index) x += 10;
    fit(all);
    cases.push_back(all);
  }
  // ---- rows
  {
    Case e = make_case("rows/leading-trailing-empty", 0, 0, 0, 64, 64);
    for (int r = 0; r < 600; ++r) {
      if (r >= 100 && r < 500)
        for (uint64_t i = rnd() % 5; i > 0; --i) {
          e.index.push_back(rnd() % 64);
          e.value.push_back(rnd());
        }
      e.offset.push_back(e.index.size());
    }
    fit(e);
    cases.push_back(e);
    // 10000 empty rows between two entries of one tile: the offsets of the tile's rows do not fit the LDS span
    Case g = make_case("rows/10000-empty-inside-a-tile", 0, 0, 0, 64, 64);
    for (int r = 0; r < 10300; ++r) {
      if (r < 150 || r >= 10150)
        for (uint64_t i = 1 + rnd() % 3; i > 0; --i) {
          g.index.push_back(rnd() % 64);
          g.value.push_back(rnd());
        }
      g.offset.push_back(g.index.size());
    }
    fit(g);
    cases.push_back(g);
    // one row of 3T + 5 entries among empty rows: tiles inside a single row
    Case l = make_case("rows/one-long-row", 0, 0, 0, 257, 257);
    for (int r = 0; r < 300; ++r) {
      if (r == 77)
        for (uint64_t i = 0; i < 3 * T + 5; ++i) {
          l.index.push_back(rnd() % 257);
          l.value.push_back(rnd());
        }
      l.offset.push_back(l.index.size());
    }
    fit(l);
    cases.push_back(l);
  }
  // ---- row windows
  {
    const Case base = make_case("window", 3000, 0, 7, 300, 303);
    Case a = base;
    a.name = "window/begin-inside-a-tile";
    a.row_begin = 1234;
    fit(a);
    cases.push_back(a);
    Case b = base;
    b.name = "window/max-rows-cuts-a-tile";
    b.row_begin = 17;
    b.max_rows = 1500;
    fit(b);
    cases.push_back(b);
    Case z = base;
    z.name = "window/max-rows-0";
    z.max_rows = 0;
    fit(z);
    cases.push_back(z);
    Case p = base;
    p.name = "window/begin-past-rows";
    p.row_begin = 3000;
    fit(p);
    cases.push_back(p);
    Case q = base;
    q.name = "window/row-cap-below-count";
    fit(q);
    q.cap_rows = 2000;
    cases.push_back(q);
    Case m = base;
    m.name = "window/max-entries-bound";
    m.row_begin = 100;
    m.max_rows = 1000;
    fit(m);
    m.max_entries = m.offset[1100] - m.offset[100] + 5;
    cases.push_back(m);
    Case s = m;
    s.name = "window/max-entries-too-small";
    s.max_entries = m.offset[1100] - m.offset[100] - 9;
    cases.push_back(s);
  }
  // ---- arrays that are not there
  {
    Case n = make_case("absent/no-values", 500, 0, 7, 300, 303, false);
    fit(n);
    cases.push_back(n);
    Case p = make_case("absent/no-pos", 500, 0, 7, 70000, 70003);
    fit(p);
    p.want_pos = false;
    cases.push_back(p);
    Case v = make_case("absent/no-value-output", 500, 0, 7, 300, 303);
    fit(v);
    v.want_val = false;
    cases.push_back(v);
  }
  // ---- capacity and flags
  {
    Case c = make_case("cap/one-short", 900, 0, 7, 300, 300);
    fit(c);
    c.out_cap -= 1;
    cases.push_back(c);
    Case c2 = make_case("cap/far-short-two-passes", 900, 0, 7, 3000, 3000);
    fit(c2);
    c2.out_cap /= 3;
    cases.push_back(c2);
    Case e = make_case("flag/error", 50, 0, 5, 300, 300);
    fit(e);
    e.res[8] = (123ull << 16) | 3;
    cases.push_back(e);
    Case f = make_case("flag/value-count", 50, 1, 5, 3000, 3000);
    fit(f);
    f.res[C_VALUE] = f.res[C_INDEX] - 1;
    cases.push_back(f);
    // offsets past the index capacity: the arrays' tail past it must not reach the output
    Case o = make_case("flag/offset-cap", 400, 1, 5, 300, 300);
    fit(o);
    o.cap_index = o.offset[250] - 2;
    for (size_t i = o.cap_index; i < o.index.size(); ++i) o.index[i] = 7, o.value[i] = 0xBADBADBADBADull;
    cases.push_back(o);
    Case o2 = make_case("flag/offset-cap-value", 400, 1, 5, 300, 300);
    fit(o2);
    o2.cap_value = o2.offset[100] + 1;
    cases.push_back(o2);
  }

  std::vector<Job *> jobs;
  for (const Case &c : cases)
    for (int combo = 0; combo < 4; ++combo) {
      const int wide = combo & 1, v8 = combo >> 1;
      // every width for the small case groups, the narrowest and the widest for the others
      const bool small = c.name.rfind("count/", 0) == 0 || c.name.rfind("drop/", 0) == 0 || c.name.rfind("absent/", 0) == 0 ||
                         c.name.rfind("cap/", 0) == 0 || c.name.rfind("flag/", 0) == 0;
      if ((c.one_width || !small) && combo != 0 && combo != 3) continue;
      if (c.single && combo != 0) continue;
      if (c.wide_only && !wide) continue;
      jobs.push_back(make_job(c, wide, v8 ? 8 : 4));
    }

  Barrier bar(kThreads);
  Barrier wbar[kWaves] = {Barrier(kWave), Barrier(kWave), Barrier(kWave), Barrier(kWave)};
  static unsigned char scan[kThreads * 64], votes[kThreads];
  static uint32_t cnt[kWaves * kCscDigits], span[kCscSpan + 1];
  static uint64_t ends[2];
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      HostBlk bk{t, &bar, wbar, scan, votes};
      for (Job *j : jobs) {
        CscArgs a = j->a;
        auto lds = [&] {  // LDS is uninitialised on the GPU
          bar.wait();
          if (t == 0) {
            std::memset(cnt, 0xCD, sizeof(cnt));
            std::memset(span, 0xCD, sizeof(span));
            std::memset(ends, 0xCD, sizeof(ends));
          }
          bar.wait();
        };
        for (a.pass = 0; a.pass < a.passes; ++a.pass) {
          for (uint64_t tile = 0; tile < a.ntiles; ++tile) {
            lds();
            if (j->wide) csc_hist_tile<uint64_t>(a, tile, cnt, bk);
            else csc_hist_tile<uint32_t>(a, tile, cnt, bk);
          }
          bar.wait();
          for (uint32_t d = 0; d < kCscDigits; ++d) csc_scan(a, d, bk);  // (the body's scans end in a barrier)
          for (uint64_t tile = 0; tile < a.ntiles; ++tile) {
            lds();
            if (j->wide) {
              if (j->vbytes == 8) csc_scatter_tile<uint64_t, uint64_t>(a, tile, cnt, span, ends, bk);
              else csc_scatter_tile<uint64_t, uint32_t>(a, tile, cnt, span, ends, bk);
            } else {
              if (j->vbytes == 8) csc_scatter_tile<uint32_t, uint64_t>(a, tile, cnt, span, ends, bk);
              else csc_scatter_tile<uint32_t, uint32_t>(a, tile, cnt, span, ends, bk);
            }
          }
        }
        bar.wait();
        if (a.passes > 1)
          for (uint64_t c = t; c < (a.ncol / kThreads + 1) * kThreads; c += kThreads) csc_bounds(a, c);
        bar.wait();
      }
    });
  for (auto &x : th) x.join();

  long bad = 0;
  uint64_t tiles = 0, multitile = 0, longscan = 0, dropped = 0, overflow = 0, multipass = 0, unstaged = 0;
  for (Job *j : jobs) {
    long mism = 0;
    for (size_t i = 0; i < j->co.size(); ++i) mism += j->co[i] != j->wco[i];
    for (size_t i = 0; i < j->orow.size(); ++i) mism += j->orow[i] != j->wrow[i];
    for (size_t i = 0; i < j->oval.size(); ++i) mism += j->oval[i] != j->wval[i];
    for (size_t i = 0; i < j->opos.size(); ++i) mism += j->opos[i] != j->wpos[i];
    for (int i = 0; i < 4; ++i) mism += j->status[i] != j->wstatus[i];
    std::printf("%-44s passes %u tiles %4llu kept %8llu dropped %5llu first %llx flags %2llu mismatches %ld\n", j->name.c_str(),
                j->a.passes, (unsigned long long)j->a.ntiles, (unsigned long long)j->status[0], (unsigned long long)j->status[1],
                (unsigned long long)j->status[2], (unsigned long long)j->status[3], mism);
    bad += mism;
    tiles += j->a.ntiles * j->a.passes;
    if (j->a.ntiles > 1) ++multitile;
    if (j->a.ntiles > (uint64_t)kThreads) ++longscan;
    if (j->a.passes > 1) ++multipass;
    if (j->status[1]) ++dropped;
    if (j->status[3] & 8) ++overflow;
    if (j->name.rfind("rows/10000", 0) == 0) ++unstaged;
    delete j;
  }
  std::printf("cases %zu, jobs %zu, tiles %llu, multi-tile %llu, long-scan %llu, multi-pass %llu, dropped %llu, overflow %llu, "
              "mismatches %ld\n",
              cases.size(), jobs.size(), (unsigned long long)tiles, (unsigned long long)multitile, (unsigned long long)longscan,
              (unsigned long long)multipass, (unsigned long long)dropped, (unsigned long long)overflow, bad);
  return bad != 0;
}
