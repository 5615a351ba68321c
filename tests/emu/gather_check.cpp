// TEST INFRASTRUCTURE ONLY: the three row-gather tile bodies (gather_core.h) on
// the CPU, 256 host threads per tile, for every index / value / label / id
// width, against a sequential loop that restates include/dmlc_amd.h's
// semantics.  Every dst buffer whole (the tail past the counts, the arrays that
// must stay unwritten and a guard element included), the dst result block and
// the four status words must be equal.  One line per job; the last line
// carries the totals tests/test_emu_gather.py reads.
// usage: gather_check [seed]
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "gather_core.h"

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
// the block policy: thread id, workgroup barrier, exclusive scan (DevBlockT::exclusive)
struct HostBlk {
  int t;
  Barrier *bar;
  unsigned char *scan;  // kThreads slots of 64 bytes
  int tid() const { return t; }
  void sync() { bar->wait(); }
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

enum { A_OFFSET = 0, A_LABEL, A_WEIGHT, A_QID, A_FIELD, A_INDEX, A_VALUE, A_N };
const int kSlotOf[A_N] = {C_ROWS, C_LABEL, C_WEIGHT, C_QID, C_FIELD, C_INDEX, C_VALUE};
const uint64_t kSentinel = 0xA5A5A5A5A5A5A5A5ull;

// one case, independent of the widths: every array as 64-bit patterns
struct Case {
  std::string name;
  std::vector<uint64_t> arr[A_N];
  bool present[A_N] = {true, true, false, false, false, true, true};  // the pointer is not null
  uint64_t res[16] = {0};
  std::vector<uint64_t> ids;
  uint64_t scap[8] = {0}, dcap[8] = {0};
  bool all_widths = true;
  bool wide_ids_only = false;  // holds ids >= 2^32
};

// rows of lo .. hi random entries; label always, the others as asked
Case make_case(const std::string &name, uint64_t rows, uint64_t lo, uint64_t hi, bool value = true, bool weight = false,
               bool qid = false, bool field = false) {
  Case c;
  c.name = name;
  c.present[A_WEIGHT] = weight;
  c.present[A_QID] = qid;
  c.present[A_FIELD] = field;
  c.present[A_VALUE] = value;
  c.arr[A_OFFSET].push_back(0);
  for (uint64_t r = 0; r < rows; ++r) {
    const uint64_t m = lo + (hi > lo ? rnd() % (hi - lo + 1) : 0);
    for (uint64_t i = 0; i < m; ++i) {
      c.arr[A_INDEX].push_back(rnd());
      if (value) c.arr[A_VALUE].push_back(rnd());
      if (field) c.arr[A_FIELD].push_back(rnd());
    }
    c.arr[A_OFFSET].push_back(c.arr[A_INDEX].size());
    c.arr[A_LABEL].push_back(rnd() | 1);
    if (weight) c.arr[A_WEIGHT].push_back(rnd() | 1);
    if (qid) c.arr[A_QID].push_back(rnd() | 1);
  }
  const uint64_t nnz = c.arr[A_INDEX].size();
  c.res[C_ROWS] = c.res[C_LABEL] = rows;
  c.res[C_INDEX] = nnz;
  c.res[C_VALUE] = value ? nnz : 0;
  c.res[C_FIELD] = field ? nnz : 0;
  c.res[C_WEIGHT] = weight ? rows : 0;
  c.res[C_QID] = qid ? rows : 0;
  c.scap[C_ROWS] = rows;
  c.scap[C_INDEX] = c.scap[C_VALUE] = c.scap[C_FIELD] = nnz;
  c.scap[C_WEIGHT] = c.scap[C_QID] = rows;
  return c;
}
// dst capacities that hold the gather exactly
void fit_dst(Case &c) {
  uint64_t e = 0;
  const uint64_t rows = mn<uint64_t>(c.res[C_ROWS], c.scap[C_ROWS]);
  for (uint64_t id : c.ids)
    if (id < rows) e += c.arr[A_OFFSET][id + 1] - c.arr[A_OFFSET][id];
  c.dcap[C_ROWS] = c.dcap[C_WEIGHT] = c.dcap[C_QID] = c.ids.size();
  c.dcap[C_INDEX] = c.dcap[C_VALUE] = c.dcap[C_FIELD] = e;
}
void ids_random(Case &c, uint64_t n) {
  for (uint64_t i = 0; i < n; ++i) c.ids.push_back(rnd() % c.res[C_ROWS]);
}

struct Buf {
  std::vector<unsigned char> b;
  size_t es = 8;
  bool null = true;
  void *ptr() { return null ? nullptr : b.data(); }
  void set(size_t i, uint64_t v) { std::memcpy(b.data() + i * es, &v, es); }  // (little endian: the low bytes)
};

struct Job {
  std::string name;
  GatherArgs a;
  int wide, vbytes;
  Buf src[A_N], dst[A_N], want[A_N];
  std::vector<unsigned char> ids;
  std::vector<uint64_t> rec;
  uint64_t res[16], dres[16], wres[16], status[4], wstatus[4];
};

GatherCsr side_of(Buf *b, const uint64_t *cap) {
  GatherCsr g;
  std::memset(&g, 0, sizeof(g));
  g.offset = static_cast<uint64_t *>(b[A_OFFSET].ptr());
  g.label = b[A_LABEL].ptr();
  g.weight = static_cast<uint32_t *>(b[A_WEIGHT].ptr());
  g.qid = static_cast<uint64_t *>(b[A_QID].ptr());
  g.field = b[A_FIELD].ptr();
  g.index = b[A_INDEX].ptr();
  g.value = b[A_VALUE].ptr();
  // as capi.cpp's gather_side: a null array holds nothing, cap[ROWS] counts labels
  g.cap[C_ROWS] = g.offset ? cap[C_ROWS] : 0;
  g.cap[C_LABEL] = g.label ? g.cap[C_ROWS] : 0;
  for (int k : {A_WEIGHT, A_QID, A_FIELD, A_INDEX, A_VALUE}) g.cap[kSlotOf[k]] = b[k].null ? 0 : cap[kSlotOf[k]];
  return g;
}

// the sequential statement of the semantics, on j.want / j.wres / j.wstatus
void reference(Job &j, const Case &c) {
  const GatherArgs &a = j.a;
  uint64_t *ws = j.wstatus;
  ws[0] = ws[1] = ws[3] = 0;
  ws[2] = ~0ull;
  std::memset(j.wres, 0, sizeof(j.wres));
  if (c.res[8]) ws[3] |= 1;
  if ((c.res[C_VALUE] && c.res[C_VALUE] != c.res[C_INDEX]) || (c.res[C_FIELD] && c.res[C_FIELD] != c.res[C_INDEX])) ws[3] |= 2;
  if (ws[3]) {
    j.wres[8] = c.res[8] ? c.res[8] : 32;
    return;
  }
  const uint64_t rows = mn<uint64_t>(c.res[C_ROWS], a.src.cap[C_ROWS]);
  bool has[A_N];
  has[A_OFFSET] = has[A_INDEX] = true;
  has[A_VALUE] = c.res[C_VALUE] != 0;
  has[A_FIELD] = c.res[C_FIELD] != 0;
  for (int k : {A_LABEL, A_WEIGHT, A_QID}) has[k] = c.res[kSlotOf[k]] != 0 && c.res[kSlotOf[k]] == c.res[C_ROWS];
  uint64_t lim = ~0ull;
  for (int k : {A_INDEX, A_VALUE, A_FIELD})
    if (has[k]) lim = mn<uint64_t>(lim, a.src.cap[kSlotOf[k]]);
  auto copy = [&](int k, uint64_t di, uint64_t si, bool zero) {
    if (di >= a.dst.cap[kSlotOf[k]]) return false;
    uint64_t v = 0;
    if (!zero && si < a.src.cap[kSlotOf[k]]) std::memcpy(&v, j.src[k].b.data() + si * j.src[k].es, j.src[k].es);
    j.want[k].set(di, v);
    return true;
  };
  const uint64_t *off = reinterpret_cast<const uint64_t *>(j.src[A_OFFSET].b.data());
  uint64_t e = 0, first_over = ~0ull;
  j.want[A_OFFSET].set(0, 0);
  const uint64_t n = c.ids.size();
  for (uint64_t i = 0; i < n; ++i) {
    const uint64_t r = c.ids[i];
    bool fits = i < a.dst.cap[C_ROWS];
    if (r >= rows) {
      ++ws[1];
      ws[2] = mn<uint64_t>(ws[2], i);
    } else {
      uint64_t o0 = off[r], o1 = off[r + 1];
      if (o0 > lim || o1 > lim) ws[3] |= 4;
      o0 = mn<uint64_t>(o0, lim);
      o1 = mn<uint64_t>(o1, lim);
      for (uint64_t k = o0; k < o1; ++k, ++e)
        for (int x : {A_INDEX, A_VALUE, A_FIELD})
          if (has[x]) fits &= copy(x, e, k, false);
    }
    for (int x : {A_LABEL, A_WEIGHT, A_QID})
      if (has[x]) fits &= copy(x, i, r, r >= rows);
    if (i + 1 <= a.dst.cap[C_ROWS]) j.want[A_OFFSET].set(i + 1, e);
    if (!fits && first_over == ~0ull) first_over = i;
  }
  ws[0] = mn<uint64_t>(n, a.dst.cap[C_ROWS]);
  j.wres[C_ROWS] = n;
  j.wres[C_INDEX] = e;
  j.wres[C_VALUE] = has[A_VALUE] ? e : 0;
  j.wres[C_FIELD] = has[A_FIELD] ? e : 0;
  for (int x : {A_LABEL, A_WEIGHT, A_QID}) j.wres[kSlotOf[x]] = has[x] ? n : 0;
  if (first_over != ~0ull) {
    ws[3] |= 8;
    j.wres[8] = (first_over << 16) | 16;
  }
}

Job *make_job(const Case &c, int wide, int vbytes, int lbytes, int idwide) {
  Job *j = new Job;
  j->name = c.name + (wide ? "/u64" : "/u32") + (vbytes == 8 ? "/v8" : "/v4") + (lbytes == 8 ? "/l8" : "/l4") +
            (idwide ? "/id64" : "/id32");
  j->wide = wide;
  j->vbytes = vbytes;
  const size_t es[A_N] = {8, (size_t)lbytes, 4, 8, wide ? 8u : 4u, wide ? 8u : 4u, (size_t)vbytes};
  for (int k = 0; k < A_N; ++k) {
    // the source holds what the case lists (it may be more than the capacity says), and a guard element
    Buf &s = j->src[k];
    s.es = es[k];
    s.null = !c.present[k];
    s.b.assign((c.arr[k].size() + 1) * es[k], 0xEE);
    for (size_t i = 0; i < c.arr[k].size(); ++i) s.set(i, c.arr[k][i]);
    // the destination: its capacity (+ 1 for offset) and two guard elements, all sentinel
    Buf &d = j->dst[k];
    d.es = es[k];
    d.null = !c.present[k];
    const uint64_t cap = k == A_OFFSET ? c.dcap[C_ROWS] + 1 : (k == A_LABEL ? c.dcap[C_ROWS] : c.dcap[kSlotOf[k]]);
    d.b.assign((cap + 2) * es[k], 0xA5);
    j->want[k] = d;
  }
  j->ids.assign((c.ids.size() + 1) * (idwide ? 8 : 4), 0);
  for (size_t i = 0; i < c.ids.size(); ++i) std::memcpy(j->ids.data() + i * (idwide ? 8 : 4), &c.ids[i], idwide ? 8 : 4);
  std::memcpy(j->res, c.res, sizeof(j->res));
  GatherArgs &a = j->a;
  std::memset(&a, 0, sizeof(a));
  a.src = side_of(j->src, c.scap);
  a.dst = side_of(j->dst, c.dcap);
  a.res = j->res;
  a.dres = j->dres;
  a.ids = j->ids.data();
  a.n_ids = c.ids.size();
  a.ntiles = (a.n_ids + kGatherRows - 1) / kGatherRows;
  a.id_wide = idwide;
  a.label_bytes = lbytes;
  j->rec.assign(a.ntiles * kGatherRecWords + 1, kSentinel);
  a.rec = j->rec.data();
  a.status = j->status;
  for (int k = 0; k < 16; ++k) j->dres[k] = kSentinel;
  for (int k = 0; k < 4; ++k) j->status[k] = kSentinel;
  reference(*j, c);
  return j;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  const uint64_t R = kGatherRows;
  std::vector<Case> cases;
  // ---- n_ids around the tile size, over rows of 0 .. 9 entries with every array
  for (uint64_t n : {(uint64_t)0, (uint64_t)1, R - 1, R, R + 1, 2 * R + 1}) {
    Case c = make_case("nids/" + std::to_string(n), 300, 0, 9, true, true, true, true);
    ids_random(c, n);
    fit_dst(c);
    cases.push_back(c);
  }
  // ---- 257 R + 3 ids over rows of 0 .. 3 entries: the scan's per-thread run is 2 tiles
  {
    Case c = make_case("scanrun/257R+3", 1000, 0, 3, true, false, true, false);
    ids_random(c, 257 * R + 3);
    fit_dst(c);
    c.all_widths = false;
    cases.push_back(c);
  }
  // ---- all rows empty; one long row among empty ones; odd lengths
  {
    Case c = make_case("empty/all", 3 * R, 0, 0);
    ids_random(c, 2 * R + 5);
    fit_dst(c);
    cases.push_back(c);
    Case l = make_case("longrow/12289-among-empty", 0, 0, 0);
    for (int r = 0; r < 400; ++r) {
      if (r == 77)
        for (int i = 0; i < 3 * 256 * 16 + 1; ++i) {
          l.arr[A_INDEX].push_back(rnd());
          l.arr[A_VALUE].push_back(rnd());
        }
      l.arr[A_OFFSET].push_back(l.arr[A_INDEX].size());
      l.arr[A_LABEL].push_back(rnd());
    }
    l.res[C_ROWS] = l.res[C_LABEL] = l.scap[C_ROWS] = 400;
    l.res[C_INDEX] = l.res[C_VALUE] = l.scap[C_INDEX] = l.scap[C_VALUE] = l.arr[A_INDEX].size();
    for (uint64_t i = 0; i < 300; ++i) l.ids.push_back(i == 140 || i == 290 ? 77 : (i * 7) % 400 == 77 ? 78 : (i * 7) % 400);
    fit_dst(l);
    cases.push_back(l);
    Case o = make_case("odd/1-3-5-7", 0, 0, 0, true, true, false, true);
    for (int r = 0; r < 500; ++r) {
      for (int i = 0; i < 1 + 2 * (r % 4); ++i) {
        o.arr[A_INDEX].push_back(rnd());
        o.arr[A_VALUE].push_back(rnd());
        o.arr[A_FIELD].push_back(rnd());
      }
      o.arr[A_OFFSET].push_back(o.arr[A_INDEX].size());
      o.arr[A_LABEL].push_back(rnd());
      o.arr[A_WEIGHT].push_back(rnd());
    }
    o.res[C_ROWS] = o.res[C_LABEL] = o.res[C_WEIGHT] = o.scap[C_ROWS] = o.scap[C_WEIGHT] = 500;
    o.res[C_INDEX] = o.res[C_VALUE] = o.res[C_FIELD] = o.scap[C_INDEX] = o.scap[C_VALUE] = o.scap[C_FIELD] = o.arr[A_INDEX].size();
    ids_random(o, R + 40);
    fit_dst(o);
    cases.push_back(o);
  }
  // ---- orders: identity, reversed, a permutation, one id repeated, a subset
  {
    const Case base = make_case("order", 2 * R + 9, 0, 6, true, true, true, false);
    const uint64_t rows = base.res[C_ROWS];
    Case c = base;
    c.name = "order/identity";
    for (uint64_t i = 0; i < rows; ++i) c.ids.push_back(i);
    fit_dst(c);
    cases.push_back(c);
    Case r = base;
    r.name = "order/reversed";
    for (uint64_t i = 0; i < rows; ++i) r.ids.push_back(rows - 1 - i);
    fit_dst(r);
    cases.push_back(r);
    Case p = c;
    p.name = "order/permutation";
    for (uint64_t i = rows - 1; i > 0; --i) std::swap(p.ids[i], p.ids[rnd() % (i + 1)]);
    cases.push_back(p);
    Case d = base;
    d.name = "order/repeated";
    for (uint64_t i = 0; i < R + 3; ++i) d.ids.push_back(i % 3 ? 5 : i);
    fit_dst(d);
    cases.push_back(d);
    Case s = base;
    s.name = "order/subset";
    for (uint64_t i = 0; i < rows; i += 3) s.ids.push_back(i);
    fit_dst(s);
    cases.push_back(s);
  }
  // ---- bad ids: rows, rows + 1, and 2^32 + 1 (64-bit ids: not wrapped to row 1)
  {
    Case b = make_case("bad/rows,rows+1", 300, 0, 5, true, true, true, true);
    ids_random(b, R + 20);
    b.ids[3] = 300;
    b.ids[R + 1] = 301;
    b.ids[200] = 300;
    fit_dst(b);
    cases.push_back(b);
    Case w = b;
    w.name = "bad/2^32+1";
    w.ids[2] = (1ull << 32) + 1;
    w.wide_ids_only = true;
    fit_dst(w);
    cases.push_back(w);
    Case z = make_case("bad/all", 10, 1, 3);
    for (uint64_t i = 0; i < R + 1; ++i) z.ids.push_back(10 + i);
    fit_dst(z);
    cases.push_back(z);
  }
  // ---- arrays that are not there: no values, no weight / qid, field; counts that differ from the rows
  {
    Case c = make_case("absent/novalue-qid", 300, 0, 5, false, false, true, false);
    ids_random(c, R + 7);
    fit_dst(c);
    cases.push_back(c);
    Case p = make_case("absent/plain", 300, 0, 5, true, false, false, false);
    ids_random(p, R + 7);
    fit_dst(p);
    cases.push_back(p);
    Case f = make_case("absent/field", 300, 0, 5, true, true, false, true);
    ids_random(f, R + 7);
    fit_dst(f);
    cases.push_back(f);
    // a weight count below the rows (libsvm rows without a weight): the array is not copied; the pointers are there
    Case w = make_case("absent/weight-count-short", 300, 0, 5, true, true, true, false);
    w.res[C_WEIGHT] = 299;
    w.res[C_LABEL] = 0;
    ids_random(w, R + 7);
    fit_dst(w);
    cases.push_back(w);
  }
  // ---- each dst capacity one short in turn
  for (int slot : {C_ROWS, C_INDEX, C_VALUE, C_FIELD, C_WEIGHT, C_QID}) {
    Case c = make_case("cap/" + std::to_string(slot) + "-one-short", 300, 1, 5, true, true, true, true);
    ids_random(c, R + 30);
    fit_dst(c);
    c.dcap[slot] -= 1;
    cases.push_back(c);
  }
  {
    Case c = make_case("cap/index-far-short", 300, 1, 5, true, true, true, true);
    ids_random(c, 2 * R + 30);
    fit_dst(c);
    c.dcap[C_INDEX] = c.dcap[C_INDEX] / 3;  // the first tile overflows; the value capacity holds everything
    cases.push_back(c);
  }
  // ---- flags
  {
    Case f = make_case("flag/value-count", 50, 0, 5);
    f.res[C_VALUE] = f.res[C_INDEX] - 1;
    ids_random(f, 40);
    fit_dst(f);
    cases.push_back(f);
    Case g = make_case("flag/field-count", 50, 1, 5, true, false, false, true);
    g.res[C_FIELD] = g.res[C_INDEX] + 1;
    ids_random(g, 40);
    fit_dst(g);
    cases.push_back(g);
    Case e = make_case("flag/error", 50, 0, 5);
    e.res[8] = (123ull << 16) | 3;
    ids_random(e, 40);
    fit_dst(e);
    cases.push_back(e);
    // offsets past the index capacity: the arrays' tail past it must not reach dst
    Case o = make_case("flag/offset-cap", 400, 1, 5, true, false, false, true);
    for (uint64_t i = 0; i < 400; ++i) o.ids.push_back(399 - i);
    o.scap[C_INDEX] = o.arr[A_OFFSET][250] - 2;
    for (size_t i = o.scap[C_INDEX]; i < o.arr[A_INDEX].size(); ++i) o.arr[A_INDEX][i] = o.arr[A_VALUE][i] = o.arr[A_FIELD][i] = 0xBADBADBADBADull;
    o.dcap[C_ROWS] = 400;
    o.dcap[C_INDEX] = o.dcap[C_VALUE] = o.dcap[C_FIELD] = o.arr[A_INDEX].size();
    cases.push_back(o);
    // a source row capacity below the row count: ids at or past it are bad
    Case r = make_case("flag/row-cap", 300, 0, 5);
    r.scap[C_ROWS] = 200;
    ids_random(r, R + 9);
    fit_dst(r);
    cases.push_back(r);
  }

  // ---- jobs: every case for every width combination
  std::vector<Job *> jobs;
  for (const Case &c : cases)
    for (int combo = 0; combo < 16; ++combo) {
      const int wide = combo & 1, v8 = (combo >> 1) & 1, l8 = (combo >> 2) & 1, id64 = (combo >> 3) & 1;
      if (!c.all_widths && combo != 0 && combo != 15) continue;
      if (c.wide_ids_only && !id64) continue;
      jobs.push_back(make_job(c, wide, v8 ? 8 : 4, l8 ? 8 : 4, id64));
    }

  Barrier bar(kThreads);
  static unsigned char scan[kThreads * 64];
  static uint64_t dpos[kGatherRows + 1], spos[kGatherRows];
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t)
    th.emplace_back([&, t] {
      HostBlk bk{t, &bar, scan};
      for (Job *j : jobs) {
        const GatherArgs &a = j->a;
        for (uint64_t tile = 0; tile < a.ntiles; ++tile) gather_lengths_tile(a, tile, bk);
        bar.wait();
        gather_scan(a, bk);
        bar.wait();
        for (uint64_t tile = 0; tile < a.ntiles; ++tile) {
          if (t == 0) {  // LDS is uninitialised on the GPU
            std::memset(dpos, 0xCD, sizeof(dpos));
            std::memset(spos, 0xCD, sizeof(spos));
          }
          bar.wait();
          if (j->wide) {
            if (j->vbytes == 8) gather_copy_tile<uint64_t, uint64_t>(a, tile, dpos, spos, bk);
            else gather_copy_tile<uint64_t, uint32_t>(a, tile, dpos, spos, bk);
          } else {
            if (j->vbytes == 8) gather_copy_tile<uint32_t, uint64_t>(a, tile, dpos, spos, bk);
            else gather_copy_tile<uint32_t, uint32_t>(a, tile, dpos, spos, bk);
          }
          bar.wait();
        }
      }
    });
  for (auto &x : th) x.join();

  long bad = 0;
  uint64_t tiles = 0, multitile = 0, badids = 0, overflow = 0, longscan = 0;
  for (Job *j : jobs) {
    long mism = 0;
    for (int k = 0; k < A_N; ++k)
      for (size_t i = 0; i < j->dst[k].b.size(); ++i) mism += j->dst[k].b[i] != j->want[k].b[i];
    for (int i = 0; i < 16; ++i) mism += j->dres[i] != j->wres[i];
    for (int i = 0; i < 4; ++i) mism += j->status[i] != j->wstatus[i];
    std::printf("%-52s tiles %4llu rows %6llu entries %7llu bad %4llu flags %2llu error %llx mismatches %ld\n", j->name.c_str(),
                (unsigned long long)j->a.ntiles, (unsigned long long)j->status[0], (unsigned long long)j->dres[C_INDEX],
                (unsigned long long)j->status[1], (unsigned long long)j->status[3], (unsigned long long)j->dres[8], mism);
    bad += mism;
    tiles += j->a.ntiles;
    if (j->a.ntiles > 1) ++multitile;
    if (j->a.ntiles > (uint64_t)kThreads) ++longscan;
    if (j->status[1]) ++badids;
    if (j->status[3] & 8) ++overflow;
    delete j;
  }
  std::printf("cases %zu, jobs %zu, tiles %llu, multi-tile %llu, long-scan %llu, bad-ids %llu, overflow %llu, mismatches %ld\n",
              cases.size(), jobs.size(), (unsigned long long)tiles, (unsigned long long)multitile, (unsigned long long)longscan,
              (unsigned long long)badids, (unsigned long long)overflow, bad);
  return bad != 0;
}
