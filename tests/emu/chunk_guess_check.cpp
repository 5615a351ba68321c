// TEST INFRASTRUCTURE ONLY: the one-trip chunk list of the single-pass tile
// prologue (fast_common.h chunk_guess_begin / chunk_guess_end) on one
// emulated wave, for every tile of synthetic unit-start tables, against
//   - a plain linear scan of cs (what the fields mean), and
//   - the search form chunk_list(), field for field (toomany tiles included,
//     whose cnext only the search's window defines);
// and the computed decoder tables (init_dec_tables) against kDecTables byte
// for byte.  Only n and cs matter to the chunk list: no text is made.
// usage: chunk_guess_check [seed]
#include <algorithm>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "fast_common.h"

using namespace dmlc_amd;
using namespace dmlc_amd::fast;

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

struct WaveCtx {
  Barrier bar{kWave};
  unsigned char bal[kWave];
  uint64_t sh8[kWave];
};
struct WaveBlk {  // the block policy's wave operations, one wave
  int t;
  WaveCtx *ctx;
  int tid() const { return t; }
  void wave_sync() { ctx->bar.wait(); }
  uint64_t ballot(bool p) {
    ctx->bal[t] = p;
    wave_sync();
    uint64_t m = 0;
    for (int i = 0; i < kWave; ++i) m |= (uint64_t)(ctx->bal[i] != 0) << i;
    wave_sync();
    return m;
  }
  template <typename T>
  T shfl(T v, int src) {
    static_assert(sizeof(T) <= 8, "shfl element");
    std::memcpy(&ctx->sh8[t], &v, sizeof(T));
    wave_sync();
    T r;
    std::memcpy(&r, &ctx->sh8[src], sizeof(T));
    wave_sync();
    return r;
  }
};

uint64_t st = 88172645463325252ull;
uint64_t rnd() {
  st ^= st << 13;
  st ^= st >> 7;
  st ^= st << 17;
  return st;
}

struct Case {
  std::string name;
  uint64_t n;
  std::vector<uint64_t> cs;     // nchunk + 1 entries, cs[0] == 0, cs[nchunk] == n, ascending
  std::vector<uint32_t> tiles;  // tiles to run
  int want_guess;               // 1: every tile from the window, 0: some tile by the search, -1: either
  uint64_t guessed = 0, searched = 0, toomany = 0, reloads = 0;
};

// the first and last tiles, about `some` spread over the text (0: every tile), and those around tile `mid`
// (one emulated tile costs some forty 64-thread barriers: the tables are many, the tiles of each few)
void pick_tiles(Case &c, uint32_t some, uint32_t mid) {
  const uint32_t nt = (uint32_t)((c.n + kTile - 1) / kTile);
  const uint32_t step = some && nt > some ? nt / some : 1;
  for (uint32_t k = 0; k < nt; ++k)
    if (k % step == 0 || k < 2 || k + 2 >= nt || (k + 1 >= mid && k <= mid + 1)) c.tiles.push_back(k);
}
Case from_starts(const std::string &name, uint64_t n, std::vector<uint64_t> s, int want, uint32_t some = 10,
                 uint32_t mid = ~0u - 1) {
  Case c;
  c.name = name;
  c.n = n;
  c.cs = std::move(s);
  c.cs.push_back(n);
  c.want_guess = want;
  pick_tiles(c, some, mid);
  return c;
}
// nchunk near-equal units over n bytes (jit: each start moved back by up to jit bytes, a cut after a newline)
std::vector<uint64_t> equal_units(uint64_t n, int nchunk, uint64_t jit) {
  std::vector<uint64_t> s;
  for (int i = 0; i < nchunk; ++i) {
    uint64_t x = (uint64_t)((__uint128_t)n * i / nchunk);
    if (i && jit) {
      const uint64_t j = rnd() % (jit + 1);
      if (j < x - s.back()) x -= j;
    }
    s.push_back(i ? (x > s.back() ? x : s.back()) : 0);
  }
  return s;
}

struct Expect {  // the linear scan
  uint64_t cfloor, cnext;
  uint32_t c_first, ncs, toomany;
  std::vector<uint64_t> csl;
  uint64_t c0;
};
Expect scan(const Case &c, uint64_t tlo, uint64_t thi) {
  const int nchunk = (int)c.cs.size() - 1;
  Expect e;
  uint64_t c0 = 0;
  for (int i = 0; i < nchunk; ++i)
    if (c.cs[i] <= tlo) c0 = (uint64_t)i;
  e.c0 = c0;
  e.cfloor = c.cs[c0];
  e.c_first = (uint32_t)c0 + (c.cs[c0] < tlo ? 1u : 0u);
  uint32_t all = 0;
  for (int i = (int)e.c_first; i < nchunk && c.cs[i] <= thi; ++i) ++all;
  e.toomany = all > (uint32_t)kMaxCs;
  e.ncs = e.toomany ? (uint32_t)kMaxCs : all;
  for (uint32_t i = 0; i < e.ncs; ++i) e.csl.push_back(c.cs[e.c_first + i]);
  e.cnext = c.cs[e.c_first + all];  // (<= nchunk: the entry after the list; the search's window decides when toomany)
  return e;
}

}  // namespace

int main(int argc, char **argv) {
  if (argc > 1) st ^= (uint64_t)atoll(argv[1]) * 0x9E3779B97F4A7C15ull;
  long bad = 0;
  // ---- decoder tables
  for (int first : {0, kFThreads - kWave, 7}) {
    DecTables tb;
    std::memset(&tb, 0xCD, sizeof(tb));
    struct Blk {
      int t;
      int tid() const { return t; }
    };
    for (int t = 0; t < kFThreads + 64; ++t) {
      Blk b{t};
      init_dec_tables(tb, b, first);
    }
    if (std::memcmp(&tb, &kDecTables, sizeof(tb)) != 0) {
      ++bad;
      std::printf("dec tables differ from kDecTables (first %d)\n", first);
    }
  }
  static_assert(sizeof(DecTables) == (16 + 16 + 9) * 8, "no padding: memcmp compares the entries");
  std::printf("dec tables: %zu bytes equal to kDecTables\n", sizeof(DecTables));

  // ---- unit-start tables
  std::vector<Case> cases;
  const uint64_t T = kTile;
  for (int nchunk : {1, 2, 63, 64, 65, 257, 5000}) {
    // equal units: >= 2 tiles each except at 5000 (3 per tile), uneven text end
    const uint64_t n = nchunk == 5000 ? 5000ull * 5461 + 77 : (uint64_t)nchunk * (2 * T + 1000) + 123;
    const int want = nchunk < 64 ? -1 : 1;  // (below 64 units the found unit may sit in the last lanes: the reload)
    cases.push_back(from_starts("equal/" + std::to_string(nchunk), n, equal_units(n, nchunk, 0), want));
    cases.push_back(from_starts("cut/" + std::to_string(nchunk), n, equal_units(n, nchunk, 300), want));
    // random units (sorted random starts, repeats -- empty units -- among them)
    std::vector<uint64_t> r{0};
    for (int i = 1; i < nchunk; ++i) r.push_back(rnd() % 4 == 0 ? r[rnd() % r.size()] : rnd() % n);
    std::sort(r.begin(), r.end());
    cases.push_back(from_starts("random/" + std::to_string(nchunk), n, r, -1));
  }
  for (int nchunk : {65, 257, 5000}) {
    // one unit holding 90 % of the text, then tiny ones: the guess misses by more than a window
    const uint64_t n = 40 * T + 999, big = n / 10 * 9;
    std::vector<uint64_t> s{0};
    for (int i = 1; i < nchunk; ++i) s.push_back(big + (uint64_t)((__uint128_t)(n - big) * (i - 1) / (nchunk - 1)));
    cases.push_back(from_starts("big-first/" + std::to_string(nchunk), n, s, 0));
    // and the mirror: tiny units, then one holding the last 90 %
    std::vector<uint64_t> m;
    for (int i = 0; i < nchunk; ++i) m.push_back((uint64_t)((__uint128_t)(n - big) * i / nchunk));
    cases.push_back(from_starts("big-last/" + std::to_string(nchunk), n, m, 0));
  }
  for (int extra : {0, 300}) {
    // one-line units: tile 5 holds exactly kMaxCs starts in [tlo, thi], tile 7 kMaxCs + 1 (toomany), tile 9
    // kMaxCs with the last at thi, tile 11 kMaxCs + 1 with the last at thi; `extra` units spread elsewhere
    const uint64_t n = 24 * T + 5;
    std::vector<uint64_t> s{0};
    for (int i = 1; i <= extra; ++i) s.push_back(12 * T + (uint64_t)((__uint128_t)(12 * T) * i / (extra + 1)));
    auto line_units = [&](uint64_t k, int cnt, bool to_thi) {
      for (int i = 0; i < cnt; ++i) s.push_back(k * T + 100 + 37 * (uint64_t)i);
      if (to_thi) s.back() = (k + 1) * T;
    };
    line_units(5, kMaxCs, false);
    line_units(7, kMaxCs + 1, false);
    line_units(9, kMaxCs, true);
    line_units(11, kMaxCs + 1, true);
    std::sort(s.begin(), s.end());
    cases.push_back(from_starts("lines/" + std::to_string(extra), n, s, -1, 0));
  }
  {
    // the same below 64 units (the whole table is the window): tile 3 holds kMaxCs + 1 starts
    std::vector<uint64_t> s{0};
    for (int i = 0; i <= kMaxCs; ++i) s.push_back(3 * T + 64 * (uint64_t)i);
    cases.push_back(from_starts("lines/small", 6 * T + 1, s, -1, 0));
  }
  for (int nchunk : {5, 70, 257}) {
    // unit starts at tlo - 1, tlo, thi - 1 and thi of a tile, one at a time and together
    const uint64_t n = (uint64_t)nchunk * 3 * T + 17;
    for (int which = 0; which < 5; ++which) {
      std::vector<uint64_t> s = equal_units(n, nchunk - 4, 0);
      const uint64_t k = (uint64_t)nchunk + 1, tlo = k * T, thi = tlo + T;
      const uint64_t at[4] = {tlo - 1, tlo, thi - 1, thi};
      for (int j = 0; j < 4; ++j) s.push_back(which == 4 || which == j ? at[j] : at[j] + 4 * T + 50 * (uint64_t)j + 9);
      std::sort(s.begin(), s.end());
      cases.push_back(from_starts("edges/" + std::to_string(nchunk) + "/" + std::to_string(which), n, s, nchunk < 64 ? -1 : 1, 6,
                                  (uint32_t)k));
    }
  }
  {
    // a found unit in the window's last lanes (c0 - lo > kWave - kMaxCs - 2): chunk_list_end reloads at c0.
    // 60 units: one window, tiles past unit 30; 200 units bunched so that the estimate falls 40 short
    const uint64_t n = 60 * 2 * T + 11;
    cases.push_back(from_starts("last-lanes/60", n, equal_units(n, 60, 0), 0, 16));
    std::vector<uint64_t> s;
    const uint64_t n2 = 200 * T;
    for (int i = 0; i < 200; ++i) s.push_back(i < 80 ? (uint64_t)i * (T / 2) : 40 * T + (uint64_t)(i - 80) * (160 * T / 120));
    cases.push_back(from_starts("last-lanes/200", n2, s, 0, 16));
  }

  WaveCtx ctx;
  TileCommon *A = new TileCommon, *B = new TileCommon;
  std::vector<std::thread> th;
  // every lane walks the same case / tile sequence; lane 0 prepares and compares between wave barriers
  for (int t = 0; t < kWave; ++t)
    th.emplace_back([&, t] {
      WaveBlk bk{t, &ctx};
      for (Case &c : cases) {
        const int nchunk = (int)c.cs.size() - 1;
        for (uint32_t k : c.tiles) {
          const uint64_t tlo = (uint64_t)k * kTile, thi = mn<uint64_t>(tlo + kTile, c.n);
          if (t == 0) {
            std::memset((void *)A, 0xCD, sizeof(*A));  // LDS is uninitialised on the GPU
            std::memset((void *)B, 0xCD, sizeof(*B));
          }
          bk.wave_sync();
          ChunkProbe p = chunk_guess_begin(c.cs.data(), nchunk, c.n, tlo, bk);
          chunk_guess_end(c.cs.data(), nchunk, tlo, thi, p, (k & 1u) != 0, *A, bk);
          chunk_list(c.cs.data(), nchunk, tlo, thi, *B, bk);
          bk.wave_sync();
          if (t == 0) {
            const Expect e = scan(c, tlo, thi);
            bool ok = A->cfloor == e.cfloor && A->c_first == e.c_first && A->ncs == e.ncs && A->toomany == e.toomany &&
                      A->bad == 0 && (e.toomany || A->cnext == e.cnext);
            for (uint32_t i = 0; ok && i < e.ncs; ++i) ok = A->csl[i] == e.csl[i];
            const bool same = A->cfloor == B->cfloor && A->cnext == B->cnext && A->c_first == B->c_first &&
                              A->ncs == B->ncs && A->toomany == B->toomany && A->bad == B->bad &&
                              std::memcmp(A->csl, B->csl, sizeof(A->csl)) == 0;  // (entries past ncs: untouched in both)
            if (!ok || !same) {
              if (bad++ < 20)
                std::printf("%s tile %u: %s (c_first %u/%u/%u ncs %u/%u/%u cnext %llu/%llu/%llu toomany %u/%u/%u)\n",
                            c.name.c_str(), k, !ok ? "differs from the linear scan" : "differs from chunk_list()",
                            A->c_first, B->c_first, e.c_first, A->ncs, B->ncs, e.ncs, (unsigned long long)A->cnext,
                            (unsigned long long)B->cnext, (unsigned long long)e.cnext, A->toomany, B->toomany, e.toomany);
            }
            // which way the tile went (the conditions of chunk_guess_end, from the scan)
            const bool in_win = c.cs[p.lo] <= tlo && e.c0 >= p.lo && e.c0 - p.lo <= (uint64_t)(kWave - kMaxCs - 2);
            if (in_win && !e.toomany) ++c.guessed;
            else ++c.searched;
            c.toomany += e.toomany;
            // the search's own reload: its window starts more than kWave - kMaxCs - 2 before the found unit
            if (nchunk < kWave && e.c0 > (uint64_t)(kWave - kMaxCs - 2) && !(in_win && !e.toomany)) ++c.reloads;
          }
        }
      }
    });
  for (auto &x : th) x.join();
  uint64_t tiles = 0, guessed = 0, searched = 0, toomany = 0, reloads = 0;
  for (const Case &c : cases) {
    std::printf("%-18s units %5zu tiles %4zu: window %4llu search %4llu toomany %llu\n", c.name.c_str(), c.cs.size() - 1,
                c.tiles.size(), (unsigned long long)c.guessed, (unsigned long long)c.searched,
                (unsigned long long)c.toomany);
    if (c.want_guess == 1 && c.searched != 0) {
      ++bad;
      std::printf("%s: near-uniform units, yet %llu tiles took the search\n", c.name.c_str(),
                  (unsigned long long)c.searched);
    }
    if (c.want_guess == 0 && c.searched == 0) {
      ++bad;
      std::printf("%s: no tile took the search (the case is meant to miss)\n", c.name.c_str());
    }
    tiles += c.tiles.size();
    guessed += c.guessed;
    searched += c.searched;
    toomany += c.toomany;
    reloads += c.reloads;
  }
  if (toomany == 0 || reloads == 0) {
    ++bad;
    std::printf("no toomany tile or no reload among the cases\n");
  }
  std::printf("tables %zu, tiles %llu, window %llu, search %llu, toomany %llu, reloads %llu, mismatches %ld\n", cases.size(),
              (unsigned long long)tiles, (unsigned long long)guessed, (unsigned long long)searched,
              (unsigned long long)toomany, (unsigned long long)reloads, bad);
  delete A;
  delete B;
  return bad != 0;
}
