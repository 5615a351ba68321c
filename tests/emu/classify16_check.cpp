// TEST INFRASTRUCTURE ONLY: the per-unit piece classifier of the single-pass
// front half (fast_common.h classify16_lut) and the quad exchange that turns
// four lanes' pieces into plane words (quad_planes, in its host form over
// bk.shfl), against classify64_lut on 64-byte segments: the four words the
// lanes of a quad return must be the segment's D, G (the two digit-plane words
// gw), N and C planes.  Also the byte-a-lane form the tile's last wave uses
// for the tail (svm_fast.h front_half): the class bits of 64 bytes gathered as
// ballots are the same planes, and the post-halo's digit word equals
// classify_dword_lut's g of its four words.
// Segments: every byte value alone and at every unit offset, then random ones
// from the grammar's alphabet mixed with all 256 byte values.
// usage: classify16_check [segments] [seed]
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fast_common.h"

using namespace dmlc_amd;
using namespace dmlc_amd::fast;

namespace {

// A quad of lanes run one after another, by replay: a lane's k-th shfl can
// only depend on the results of its earlier ones, so pass p (every lane run
// from the start) has the right values sent at calls 0 .. p, and answers
// calls 0 .. p - 1 from the pass before.  quad_planes shuffles twice: three
// passes.
constexpr int kMaxCalls = 4;
struct QuadCtx {
  uint32_t sent[2][kMaxCalls][kWave];  // [pass parity][call][lane]
  int pass = 0;
};
struct QuadBlk {
  int t;
  QuadCtx *ctx;
  int call = 0;
  int tid() const { return t; }
  template <typename T>
  T shfl(T v, int src) {
    static_assert(sizeof(T) == 4, "quad_planes moves 32-bit registers");
    if (call >= kMaxCalls) abort();
    uint32_t x;
    std::memcpy(&x, &v, 4);
    ctx->sent[ctx->pass & 1][call][t & (kWave - 1)] = x;
    const uint32_t r = ctx->pass > call ? ctx->sent[(ctx->pass - 1) & 1][call][src] : 0u;
    ++call;
    T o;
    std::memcpy(&o, &r, 4);
    return o;
  }
};

uint64_t st = 88172645463325252ull;
uint64_t rnd() {
  st ^= st << 13;
  st ^= st >> 7;
  st ^= st << 17;
  return st;
}

uint32_t cls[kClsEntries];
uint64_t nseg = 0, mismatches = 0, with_hi = 0, with_letters = 0, with_outside = 0;

void fail(const char *what, const uint8_t *seg, uint64_t got, uint64_t want) {
  if (++mismatches > 20) return;
  printf("MISMATCH %s: got %016llx want %016llx, segment", what, (unsigned long long)got, (unsigned long long)want);
  for (int i = 0; i < 64; ++i) printf(" %02x", seg[i]);
  printf("\n");
}

// the segment at seg (16-byte aligned), its quad at lanes base .. base + 3 of a wave
void check(const uint8_t *seg, int base) {
  ++nseg;
  const Masks ref = classify64_lut(seg, cls);
  Piece16 p[4];
  for (int q = 0; q < 4; ++q) {
    uint32_t w[4];
    load16(seg + 16 * q, w);
    p[q] = classify16_lut(w, cls);
    // a piece is its quarter of the planes
    const uint32_t d = (uint32_t)(ref.d >> (16 * q)) & 0xFFFFu, g = (uint32_t)(ref.g >> (16 * q)) & 0xFFFFu;
    const uint32_t n = (uint32_t)(ref.n >> (16 * q)) & 0xFFFFu, c = (uint32_t)(ref.c >> (16 * q)) & 0xFFFFu;
    if (p[q].dg != (d | (g << 16))) fail("piece dg", seg, p[q].dg, d | (g << 16));
    if (p[q].nc != (n | (c << 16))) fail("piece nc", seg, p[q].nc, n | (c << 16));
  }
  QuadCtx ctx;
  uint64_t word[4] = {0, 0, 0, 0};
  for (ctx.pass = 0; ctx.pass < 3; ++ctx.pass)
    for (int j = 0; j < 4; ++j) {
      QuadBlk bk{base + j, &ctx};
      word[j] = quad_planes(p[j], bk);
      if (bk.call != 2) abort();
    }
  // planes and the two digit-plane words, as front_half stores them
  uint32_t gw[2];
  std::memcpy(gw, &word[1], 8);
  if (word[0] != ref.d) fail("plane D", seg, word[0], ref.d);
  if ((gw[0] | ((uint64_t)gw[1] << 32)) != ref.g) fail("gw", seg, word[1], ref.g);
  if (word[2] != ref.n) fail("plane N", seg, word[2], ref.n);
  if (word[3] != ref.c) fail("plane C", seg, word[3], ref.c);
  // the tail's form: a byte a lane, the class bits as ballots
  uint64_t D = 0, G = 0, N = 0, C = 0;
  for (int l = 0; l < 64; ++l) {
    const uint32_t x = cls[cls_index(seg[l])];
    D |= (uint64_t)((x & 0x00000001u) != 0u) << l;
    G |= (uint64_t)((x & 0x00000100u) != 0u) << l;
    N |= (uint64_t)((x & 0x00010000u) != 0u) << l;
    C |= (uint64_t)((x & 0x01000000u) != 0u) << l;
  }
  if (D != ref.d || G != ref.g || N != ref.n || C != ref.c) fail("ballot planes", seg, D ^ G ^ N ^ C, 0);
  // the post-halo's digit word: the first 16 bytes, classify_dword_lut's g (a byte >= 0x80 is none)
  uint32_t P = 0, want = 0;
  for (int l = 0; l < 16; ++l) P |= (uint32_t)((cls[cls_index(seg[l])] & 0x100u) != 0u && seg[l] < 0x80u) << l;
  for (int i = 0; i < 4; ++i) {
    uint32_t x;
    std::memcpy(&x, seg + 4 * i, 4);
    want |= classify_dword_lut(x, cls).g << (4 * i);
  }
  if (P != want) fail("post-halo digit word", seg, P, want);
  with_hi += hi_mask64(seg) != 0;
  with_letters += (ref.n & ref.c) != 0;
  with_outside += ref.bad != 0;
}

}  // namespace

int main(int argc, char **argv) {
  const uint64_t want = argc > 1 ? strtoull(argv[1], nullptr, 0) : (2ull << 20);
  if (argc > 2) st ^= strtoull(argv[2], nullptr, 0) * 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < kClsEntries; ++i) cls[i] = class_of((uint32_t)i);
  alignas(16) uint8_t seg[64];
  // every byte value: the whole segment, and alone among blanks at each unit offset of each quarter
  for (int v = 0; v < 256; ++v) {
    std::memset(seg, v, 64);
    check(seg, 4 * (v & 15));
    for (int pos = 0; pos < 64; ++pos) {
      std::memset(seg, ' ', 64);
      seg[pos] = (uint8_t)v;
      check(seg, 4 * (pos & 15));
    }
  }
  static const char alpha[] = "0123456789+-.eE:\n\r \tqid#0123456789:  ";
  while (nseg < want) {
    const uint64_t mix = rnd() % 5;  // 0: grammar only .. 4: every byte random
    for (int i = 0; i < 64; ++i) {
      const uint64_t r = rnd();
      seg[i] = (r >> 8) % 4 < mix ? (uint8_t)(r >> 16) : (uint8_t)alpha[(r >> 24) % (sizeof(alpha) - 1)];
    }
    check(seg, 4 * (int)(rnd() % 16));
  }
  printf("segments %llu, with a byte >= 0x80 %llu, with letters %llu, with bytes outside the grammar %llu, "
         "mismatches %llu\n",
         (unsigned long long)nseg, (unsigned long long)with_hi, (unsigned long long)with_letters,
         (unsigned long long)with_outside, (unsigned long long)mismatches);
  return mismatches ? 1 : 0;
}
