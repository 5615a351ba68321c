// TEST INFRASTRUCTURE ONLY: the quantile cuts' tile bodies (cuts_core.h) on the
// CPU, 256 host threads per tile, every launch of the sequence in order, against
// a sequential loop that restates include/dmlc_amd.h's walk.  cut_ptr whole
// (guard words past ncol + 1 included), cut_value allocated at exactly its
// capacity (a store past it is a heap overflow under ASan) and the eight status
// words must be equal.  One line per job; the last line carries the totals
// tests/test_emu_cuts.py reads.
// usage: cuts_check [seed]
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "cuts_core.h"

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
uint32_t fbits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}
// a finite float's bits: mostly from a pool of 40 values (ties), else anything finite
uint32_t rnd_value() {
  if (rnd() % 3) return fbits((float)((int)(rnd() % 40) - 20) * 0.25f);
  uint32_t b = (uint32_t)rnd();
  if ((b & 0x7F800000u) == 0x7F800000u) b &= 0xBFFFFFFFu;
  return b;
}

struct Case {
  std::string name;
  std::vector<uint64_t> offset, index;
  std::vector<uint32_t> value;  // float bits; empty = no value array
  uint64_t res[16] = {0};
  uint64_t cap_rows = 0, cap_index = 0, cap_value = 0;
  uint64_t row_begin = 0, max_rows = ~0ull, ncol = 1, max_entries = 0;
  uint32_t max_bin = 256;
  long cap_delta = 0;      // the output capacity relative to N_CUTS
  bool cap_zero = false;   // ... or none at all
  bool wide_only = false;  // holds indices >= 2^32
  bool both = false;       // run with 32- and 64-bit indices
};

// rows of lo .. hi entries with columns below `colmax`
Case make_case(const std::string &name, uint64_t rows, uint64_t lo, uint64_t hi, uint64_t ncol, uint64_t colmax,
               uint32_t max_bin = 256, bool value = true) {
  Case c;
  c.name = name;
  c.ncol = ncol;
  c.max_bin = max_bin;
  c.offset.push_back(0);
  for (uint64_t r = 0; r < rows; ++r) {
    const uint64_t m = lo + (hi > lo ? rnd() % (hi - lo + 1) : 0);
    for (uint64_t i = 0; i < m; ++i) {
      c.index.push_back(rnd() % colmax);
      if (value) c.value.push_back(rnd_value());
    }
    c.offset.push_back(c.index.size());
  }
  return c;
}
void add(Case &c, uint64_t col, uint32_t bits) {
  c.index.push_back(col);
  c.value.push_back(bits);
}
// rows of at most 7 entries over what add() listed
void rows_of(Case &c) {
  c.offset.assign(1, 0);
  while (c.offset.back() < c.index.size()) c.offset.push_back(mn<uint64_t>(c.offset.back() + 1 + rnd() % 7, c.index.size()));
  c.offset.push_back(c.index.size());  // an empty last row
}
// counts and capacities that hold the case exactly
void fit(Case &c) {
  const uint64_t rows = c.offset.size() - 1, nnz = c.index.size();
  c.res[C_ROWS] = rows;
  c.res[C_INDEX] = nnz;
  c.res[C_VALUE] = c.value.empty() ? 0 : nnz;
  c.cap_rows = rows;
  c.cap_index = nnz;
  c.cap_value = c.value.empty() ? 0 : nnz;
}

struct Job {
  std::string name;
  CutsArgs a;
  int wide;
  std::vector<unsigned char> index;
  std::vector<uint32_t> value, ptr, wptr, wval;
  std::vector<uint64_t> offset;
  uint32_t *val = nullptr;  // exactly cap words
  uint64_t *meta, *rec;     // the workspace, every part at exactly its size
  uint32_t *total, *hist, *col[2], *key[2], *cstart, *cn;
  uint64_t res[16], status[8], wstatus[8];
  bool dedupe = false;
};
const uint32_t kSentinel = 0xA5A5A5A5u;

uint32_t ref_key(uint32_t b) {
  if (b == 0x80000000u) b = 0;
  if ((b & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  return (b >> 31) ? ~b : b | 0x80000000u;
}
uint32_t ref_unkey(uint32_t k) { return (k >> 31) ? k & 0x7fffffffu : ~k; }

// the sequential statement of the semantics: all cuts, cut_ptr and the status for capacity `cap`
void reference(Job &j, const Case &c, uint64_t cap, std::vector<uint32_t> *cuts) {
  uint64_t *ws = j.wstatus;
  for (int i = 0; i < 8; ++i) ws[i] = 0;
  ws[2] = ~0ull;
  cuts->clear();
  if (c.res[8]) ws[3] |= 1;
  if (c.res[C_VALUE] && c.res[C_VALUE] != c.res[C_INDEX]) ws[3] |= 2;
  if (ws[3]) {
    for (uint64_t k = 0; k <= c.ncol; ++k) j.wptr[k] = 0;
    ws[6] = c.ncol;
    return;
  }
  const bool has_val = c.res[C_VALUE] != 0;
  const uint64_t lim = has_val ? mn<uint64_t>(c.cap_index, c.cap_value) : c.cap_index;
  const uint64_t rows = mn<uint64_t>(c.res[C_ROWS], c.cap_rows);
  const uint64_t r1 = mn<uint64_t>(rows, c.row_begin + c.max_rows < c.row_begin ? ~0ull : c.row_begin + c.max_rows);
  const uint64_t m = c.max_entries ? mn<uint64_t>(c.max_entries, c.cap_index) : c.cap_index;
  std::vector<std::pair<uint64_t, uint32_t>> ents;  // (column, key)
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
        ents.push_back({col, has_val ? ref_key(c.value[k]) : ref_key(0x3F800000u)});
      }
    }
  }
  ws[0] = ents.size();
  std::sort(ents.begin(), ents.end());
  size_t at = 0;
  const uint64_t B = c.max_bin;
  for (uint64_t col = 0; col < c.ncol; ++col) {
    j.wptr[col] = (uint32_t)cuts->size();
    const size_t lo = at;
    while (at < ents.size() && ents[at].first == col) ++at;
    size_t n = at - lo;
    while (n > 0 && ents[lo + n - 1].second == 0xffffffffu) --n, ++ws[4];
    if (n == 0) {
      ++ws[6];
      continue;
    }
    for (uint64_t i = 1; i < B; ++i) {
      const uint32_t t = ents[lo + i * n / B].second, p = ents[lo + (i - 1) * n / B].second;
      if (t > p) cuts->push_back(ref_unkey(t));
      else j.dedupe = true;
    }
    const uint32_t top = ents[lo + n - 1].second;
    const uint32_t last = ref_unkey(top == 0xff800000u ? top : top + 1);
    cuts->push_back(last == 0x80000000u ? 0u : last);
  }
  j.wptr[c.ncol] = (uint32_t)cuts->size();
  ws[5] = cuts->size();
  if (cuts->size() > cap) ws[3] |= 8;
}

Job *make_job(const Case &c, int wide) {
  Job *j = new Job;
  j->name = c.name + (wide ? "/u64" : "/u32");
  j->wide = wide;
  const size_t ib = wide ? 8 : 4;
  // the source holds what the case lists (it may be more than the capacity says), and a guard element
  j->index.assign((c.index.size() + 1) * ib, 0xEE);
  for (size_t i = 0; i < c.index.size(); ++i) std::memcpy(j->index.data() + i * ib, &c.index[i], ib);
  j->value = c.value;
  j->value.push_back(0x7FC00000u);
  j->offset = c.offset;
  std::memcpy(j->res, c.res, sizeof(j->res));
  j->ptr.assign(c.ncol + 3, kSentinel);
  j->wptr = j->ptr;
  // the capacity: relative to what the walk emits
  std::vector<uint32_t> cuts;
  reference(*j, c, ~0ull, &cuts);
  const uint64_t ncuts = cuts.size();
  uint64_t cap = c.cap_zero ? 0 : (uint64_t)mx<long>((long)ncuts + c.cap_delta, 0);
  reference(*j, c, cap, &cuts);
  j->wval.assign(cap, kSentinel);
  for (uint64_t i = 0; i < mn<uint64_t>(cap, cuts.size()); ++i) j->wval[i] = cuts[i];
  j->val = new uint32_t[cap];
  for (uint64_t i = 0; i < cap; ++i) j->val[i] = kSentinel;
  CutsArgs &a = j->a;
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
  a.ntiles = mx<uint64_t>(1, (m + kCutsTile - 1) / kCutsTile);
  a.max_bin = c.max_bin;
  a.passes = kCutsKeyPasses + cuts_col_passes(c.ncol);
  a.cut_ptr = j->ptr.data();
  a.cut_value = j->val;
  a.cap = cap;
  a.status = j->status;
  // the workspace, every word 0xCD
  auto fill32 = [](uint64_t n) {
    uint32_t *p = new uint32_t[n];
    std::memset(p, 0xCD, n * 4);
    return p;
  };
  auto fill64 = [](uint64_t n) {
    uint64_t *p = new uint64_t[n];
    std::memset(p, 0xCD, n * 8);
    return p;
  };
  a.meta = j->meta = fill64(4);
  a.total = j->total = fill32(kCutsDigits);
  a.rec = j->rec = fill64(a.ntiles * kCutsRecWords);
  a.hist = j->hist = fill32(a.ntiles * kCutsDigits);
  for (int b = 0; b < 2; ++b) {
    a.col[b] = j->col[b] = fill32(m);
    a.key[b] = j->key[b] = fill32(m);
  }
  a.cstart = j->cstart = fill32(c.ncol + 1);
  a.cn = j->cn = fill32(c.ncol);
  for (int k = 0; k < 8; ++k) j->status[k] = 0xA5A5A5A5A5A5A5A5ull;
  return j;
}
void free_job(Job *j) {
  delete[] j->val;
  delete[] j->meta;
  delete[] j->total;
  delete[] j->rec;
  delete[] j->hist;
  for (int b = 0; b < 2; ++b) {
    delete[] j->col[b];
    delete[] j->key[b];
  }
  delete[] j->cstart;
  delete[] j->cn;
  delete j;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  const uint64_t T = kCutsTile;
  std::vector<Case> cases;
  // ---- entry counts around the tile size, rows of 0 .. 9 entries
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, T - 1, T, T + 1, 2 * T + 1}) {
    Case c = make_case("count/" + std::to_string(n), 0, 0, 0, 200, 200);
    while (c.index.size() < n) {
      const uint64_t m = mn<uint64_t>(rnd() % 10, n - c.index.size());
      for (uint64_t i = 0; i < m; ++i) add(c, rnd() % 210, rnd_value());  // some at or past ncol
      c.offset.push_back(c.index.size());
    }
    if (n == 0) c.offset.assign(4, 0);
    fit(c);
    c.both = true;
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
      c.value[i] = (uint32_t)rnd() & 0x7F7FFFFFu;
      if (i % 37 == 36) c.offset.push_back(i + 1);
    }
    c.offset.push_back(n);
    fit(c);
    cases.push_back(c);
  }
  // ---- ncol and the column's pass count; empty columns first, last and in the middle
  for (uint64_t ncol : {1ull, 2ull, 255ull, 256ull, 257ull, 65536ull, 65537ull}) {
    Case c = make_case("ncol/" + std::to_string(ncol), 300, 0, 8, ncol, ncol + (ncol > 2 ? 3 : 1));
    if (ncol > 200) {  // the top columns are there
      c.index[0] = ncol - 1;
      c.index[1] = ncol - 2;
      c.index[2] = 0;
    }
    fit(c);
    cases.push_back(c);
    if (ncol < 255) continue;
    Case e = make_case("ncol-empty/" + std::to_string(ncol), 300, 0, 8, ncol, ncol);
    for (auto &x : e.index)
      if (x == 0 || x == ncol - 1 || x == ncol / 2) x = 1 + rnd() % 100;
    fit(e);
    cases.push_back(e);
  }
  // ---- max_bin, below, at and above a workgroup
  for (uint32_t B : {1u, 2u, 3u, 255u, 256u, 257u, 4096u}) {
    Case c = make_case("maxbin/" + std::to_string(B), 700, 0, 8, 5, 5, B);
    for (size_t i = 0; i < c.index.size(); ++i)
      if (c.index[i] == 3) c.value[i] = (uint32_t)rnd() & 0x7F7FFFFFu;  // a column of distinct values
    fit(c);
    cases.push_back(c);
  }
  // ---- columns of n in {1, 2, B-1, B, B+1} samples (ranks repeat when n < B), an all-equal column
  for (uint32_t B : {16u, 256u}) {
    Case c;
    c.name = "samples/B" + std::to_string(B);
    c.ncol = 8;
    c.max_bin = B;
    const uint64_t ns[] = {1, 2, B - 1, B, B + 1, 0, 3 * B + 7};
    for (uint64_t col = 0; col < 7; ++col)
      for (uint64_t i = 0; i < ns[col]; ++i) add(c, col, col == 6 ? fbits(2.5f) : (uint32_t)rnd() & 0x7F7FFFFFu);
    for (size_t i = c.index.size(); i > 1; --i) {  // shuffled
      const size_t k = rnd() % i;
      std::swap(c.index[i - 1], c.index[k]);
      std::swap(c.value[i - 1], c.value[k]);
    }
    rows_of(c);
    fit(c);
    cases.push_back(c);
  }
  // ---- a column of 3T + 5 samples among columns of one
  {
    Case c;
    c.name = "skew/3T+5-among-ones";
    c.ncol = 300;
    for (uint64_t i = 0; i < 3 * T + 5; ++i) {
      add(c, 77, rnd_value());
      if (i % 43 == 0) add(c, (i / 43) % 300 == 77 ? 78 : (i / 43) % 300, rnd_value());
    }
    rows_of(c);
    fit(c);
    cases.push_back(c);
  }
  // ---- keys that differ in exactly one byte: each of the four key passes must matter
  for (int byte = 0; byte < 4; ++byte) {
    Case c;
    c.name = "keybyte/" + std::to_string(byte);
    c.ncol = 3;
    for (int i = 0; i < 900; ++i) add(c, rnd() % 3, 0x40000000u ^ ((uint32_t)(rnd() % (byte == 3 ? 0x3F : 0x100)) << (8 * byte)));
    rows_of(c);
    fit(c);
    cases.push_back(c);
  }
  // ---- keys that tie in all four bytes across columns: the column passes must be stable over them
  for (uint64_t ncol : {300ull, 70000ull}) {
    Case c = make_case("ties/ncol" + std::to_string(ncol), 0, 0, 0, ncol, ncol, 16);
    const uint32_t pool[5] = {fbits(-3.f), fbits(-0.5f), fbits(0.f), fbits(1.f), fbits(7.f)};
    for (uint64_t i = 0; i < 2 * T + 1; ++i) add(c, (rnd() % 40) * (ncol / 40) + (rnd() % 2 ? 0 : 256 % ncol), pool[rnd() % 5]);
    rows_of(c);
    fit(c);
    cases.push_back(c);
  }
  // ---- the float edges
  for (uint32_t B : {4u, 256u}) {
    Case c;
    c.name = "special/B" + std::to_string(B);
    c.ncol = 14;
    c.max_bin = B;
    const uint32_t pz = 0, nz = 0x80000000u, pinf = 0x7F800000u, ninf = 0xFF800000u, fmax = 0x7F7FFFFFu;
    const uint32_t nan1 = 0x7FC00001u, nan2 = 0xFFC12345u, nan3 = 0x7F800001u, nan4 = 0xFFFFFFFFu;
    const std::vector<std::vector<uint32_t>> cols = {
        {nz, pz},                                   // one cut: the smallest denormal
        {fmax},                                     // last cut +inf
        {ninf},                                     // -FLT_MAX
        {pinf},                                     // +inf stays
        {ninf, pinf, fbits(1.f), fbits(-1.f)},      //
        {1u, 2u, 0x80000001u, 0x80000002u, 0x007FFFFFu, 0x807FFFFFu},  // denormals of both signs
        {0x80000001u, fbits(-1.f), fbits(-2.f)},    // the largest negative denormal on top: the +0.0 rule
        {nan1, nan2, nan3, nan4},                   // all NaN: no cuts
        {nan1, pinf, fbits(3.f), nan2},             // NaN next to +inf
        {nz, nz, nz},                               // -0.0 alone
        {},                                         // empty
        {fbits(0.f), fbits(1.f), fbits(2.f), fbits(0.f), fbits(1.f), fbits(2.f), fbits(2.f)},
        {fmax, 0xFF7FFFFFu, pinf, ninf, nan4},
        {0x00800000u, 0x80800000u, pz},             // the smallest normals around zero
    };
    for (int rep = 0; rep < 3; ++rep)
      for (size_t col = 0; col < cols.size(); ++col)
        for (uint32_t v : cols[col]) add(c, col, v);
    rows_of(c);
    fit(c);
    c.both = true;
    cases.push_back(c);
  }
  // ---- dropped entries
  {
    Case c = make_case("drop/ncol,ncol+1,2^32-1", 400, 1, 6, 100, 100);
    c.index[7] = 100;
    c.index[3] = 101;
    c.index[500] = 0xFFFFFFFFull;
    fit(c);
    c.both = true;
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
    all.both = true;
    cases.push_back(all);
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
    m.name = "window/max-entries-exact";
    m.row_begin = 100;
    m.max_rows = 1000;
    fit(m);
    m.max_entries = m.offset[1100] - m.offset[100];
    cases.push_back(m);
    Case s = m;
    s.name = "window/max-entries-one-short";
    s.max_entries = m.offset[1100] - m.offset[100] - 1;
    cases.push_back(s);
  }
  // ---- no value array: every sample is 1.0f
  {
    Case n = make_case("absent/no-values", 500, 0, 7, 300, 303, 256, false);
    fit(n);
    n.both = true;
    cases.push_back(n);
  }
  // ---- capacity and flags
  {
    Case c = make_case("cap/one-short", 900, 0, 7, 300, 300);
    fit(c);
    c.cap_delta = -1;
    c.both = true;
    cases.push_back(c);
    Case c1 = make_case("cap/two-spare", 900, 0, 7, 300, 300);
    fit(c1);
    c1.cap_delta = 2;
    cases.push_back(c1);
    Case c2 = make_case("cap/far-short", 900, 0, 7, 3000, 3000, 4096);
    fit(c2);
    c2.cap_delta = -2000;
    c2.both = true;
    cases.push_back(c2);
    Case c3 = make_case("cap/none", 200, 0, 7, 30, 30);
    fit(c3);
    c3.cap_zero = true;
    cases.push_back(c3);
    Case e = make_case("flag/error", 50, 0, 5, 300, 300);
    fit(e);
    e.res[8] = (123ull << 16) | 3;
    e.both = true;
    cases.push_back(e);
    Case f = make_case("flag/value-count", 50, 1, 5, 3000, 3000);
    fit(f);
    f.res[C_VALUE] = f.res[C_INDEX] - 1;
    f.both = true;
    cases.push_back(f);
    // offsets past the index capacity: the arrays' tail past it must not become a sample
    Case o = make_case("flag/offset-cap", 400, 1, 5, 300, 300);
    fit(o);
    o.cap_index = o.offset[250] - 2;
    for (size_t i = o.cap_index; i < o.index.size(); ++i) o.index[i] = 7, o.value[i] = fbits(1e30f);
    o.both = true;
    cases.push_back(o);
    Case o2 = make_case("flag/offset-cap-value", 400, 1, 5, 300, 300);
    fit(o2);
    o2.cap_value = o2.offset[100] + 1;
    o2.both = true;
    cases.push_back(o2);
  }

  std::vector<Job *> jobs;
  for (const Case &c : cases)
    for (int wide = 0; wide < 2; ++wide) {
      if (wide ? !(c.both || c.wide_only) : c.wide_only) continue;
      jobs.push_back(make_job(c, wide));
    }

  Barrier bar(kThreads);
  Barrier wbar[kWaves] = {Barrier(kWave), Barrier(kWave), Barrier(kWave), Barrier(kWave)};
  static unsigned char scan[kThreads * 64], votes[kThreads];
  static uint32_t cnt[kWaves * kCutsDigits], stage[2 * kCutsTile], gdelta[kCutsDigits + 1];
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      HostBlk bk{t, &bar, wbar, scan, votes};
      for (Job *j : jobs) {
        CutsArgs a = j->a;
        auto lds = [&] {  // LDS is uninitialised on the GPU
          bar.wait();
          if (t == 0) {
            std::memset(cnt, 0xCD, sizeof(cnt));
            std::memset(stage, 0xCD, sizeof(stage));
            std::memset(gdelta, 0xCD, sizeof(gdelta));
          }
          bar.wait();
        };
        for (a.pass = 0; a.pass < a.passes; ++a.pass) {
          for (uint64_t tile = 0; tile < a.ntiles; ++tile) {
            lds();
            if (j->wide) cuts_hist_tile<uint64_t>(a, tile, cnt, bk);
            else cuts_hist_tile<uint32_t>(a, tile, cnt, bk);
          }
          bar.wait();
          for (uint32_t d = 0; d < kCutsDigits; ++d) cuts_scan(a, d, bk);  // (the body's scans end in a barrier)
          bar.wait();
          for (uint64_t tile = 0; tile < a.ntiles; ++tile) {
            lds();
            if (a.pass != 0) cuts_scatter_tile<uint32_t, false>(a, tile, cnt, stage, gdelta, bk);
            else if (j->wide) cuts_scatter_tile<uint64_t, true>(a, tile, cnt, stage, gdelta, bk);
            else cuts_scatter_tile<uint32_t, true>(a, tile, cnt, stage, gdelta, bk);
          }
        }
        a.pass = a.passes;
        bar.wait();
        for (uint64_t c = t; c < (a.ncol / kThreads + 1) * kThreads; c += kThreads) cuts_bounds(a, c);
        bar.wait();
        for (uint64_t c = 0; c < a.ncol; ++c) cuts_count_col(a, c, bk);
        bar.wait();
        cuts_ptr(a, bk);
        bar.wait();
        for (uint64_t c = 0; c < a.ncol; ++c) cuts_write_col(a, c, bk);
        bar.wait();
      }
    });
  for (auto &x : th) x.join();

  long bad = 0;
  uint64_t tiles = 0, multitile = 0, longscan = 0, multipass = 0, dropped = 0, nan = 0, dedupe = 0, overflow = 0, bigbin = 0;
  for (Job *j : jobs) {
    long mism = 0;
    for (size_t i = 0; i < j->ptr.size(); ++i) mism += j->ptr[i] != j->wptr[i];
    for (size_t i = 0; i < j->wval.size(); ++i) mism += j->val[i] != j->wval[i];
    for (int i = 0; i < 8; ++i) mism += j->status[i] != j->wstatus[i];
    std::printf("%-40s passes %u tiles %4llu bin %4u kept %8llu dropped %5llu first %llx flags %2llu nan %4llu cuts %7llu "
                "empty %6llu mismatches %ld\n",
                j->name.c_str(), j->a.passes, (unsigned long long)j->a.ntiles, j->a.max_bin, (unsigned long long)j->status[0],
                (unsigned long long)j->status[1], (unsigned long long)j->status[2], (unsigned long long)j->status[3],
                (unsigned long long)j->status[4], (unsigned long long)j->status[5], (unsigned long long)j->status[6], mism);
    bad += mism;
    tiles += j->a.ntiles * j->a.passes;
    if (j->a.ntiles > 1) ++multitile;
    if (j->a.ntiles > (uint64_t)kThreads) ++longscan;
    if (j->a.passes > kCutsKeyPasses + 1) ++multipass;
    if (j->wstatus[1]) ++dropped;
    if (j->wstatus[4]) ++nan;
    if (j->dedupe) ++dedupe;
    if (j->wstatus[3] & 8) ++overflow;
    if (j->a.max_bin > (uint32_t)kThreads && j->wstatus[5]) ++bigbin;
    free_job(j);
  }
  std::printf("cases %zu, jobs %zu, tiles %llu, multi-tile %llu, long-scan %llu, multi-pass %llu, dropped %llu, nan %llu, "
              "dedupe %llu, overflow %llu, big-bin %llu, mismatches %ld\n",
              cases.size(), jobs.size(), (unsigned long long)tiles, (unsigned long long)multitile, (unsigned long long)longscan,
              (unsigned long long)multipass, (unsigned long long)dropped, (unsigned long long)nan, (unsigned long long)dedupe,
              (unsigned long long)overflow, (unsigned long long)bigbin, bad);
  return bad != 0;
}
