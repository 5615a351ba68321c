// fast_common.h -- pieces shared by the single-pass uniform-grammar kernels
// (svm_fast.h for libsvm, csv_fast.h for CSV): tile geometry, the byte-class
// tables, SWAR number decoders, LDS staging, the chunk list of a tile and the
// decoupled look-back.  Compiles as HIP device code and as plain C++ (test
// emulator, tests/emu).
#pragma once
#include "args.h"
#include "decode.h"

namespace dmlc_amd {
namespace fast {

// Tile geometry: kFThreads threads (args.h kFastThreads), 64 text bytes each.
constexpr int kFThreads = kFastThreads;
constexpr int kFWaves = kFThreads / kWave;
static_assert(kFThreads % kWave == 0 && (kFWaves == 1 || kFWaves == 2 || kFWaves == 4 || kFWaves == 6 || kFWaves == 8),
              "whole waves: 1, 2, 4, 6 or 8");

// LDS of one single-pass workgroup.  gfx950 allocates LDS in 1280-byte
// granules (160 KiB / 128): at four waves per tile, 6 workgroups per CU fit
// 21 granules each (26,880 bytes), one byte more and the launch dropped to 5
// per CU (+32 bytes took svm_fast_tile from 1.84 to 2.04 ms); a one-wave
// tile gets 6 granules (7,680 bytes: 21 workgroups per CU); six- and eight-wave
// tiles (24 / 32 KiB of text) get 4 and 3 workgroups per CU: 32 and 42 granules.
constexpr int kLdsGranule = 1280;
constexpr int kLdsBudget =
    (kFWaves == 1 ? 6 : kFWaves == 2 ? 11 : kFWaves == 4 ? 21 : kFWaves == 6 ? 32 : 42) * kLdsGranule;

constexpr int kSegB = 64;                 // bytes per thread (one 64-bit mask)
constexpr int kTile = kFThreads * kSegB;  // text per tile (4 KiB at one wave)
constexpr int kPre = 64;                  // staged bytes before the tile (the segment before it)
// (staging 80 bytes before the tile instead -- 16 more for the qid token
// checks -- cost 11 % on the 1M x 128 libsvm launch: those read global memory)
constexpr int kPost = kFWaves == 1 ? 64 : 128;  // staged bytes after it (runs crossing the end)
constexpr int kStage = kPre + kTile + kPost;
constexpr int kMaxCs = kFastMaxCs;       // chunk starts per tile the fast path accepts (args.h)
constexpr uint64_t kAgg = 1ull << 62, kIncl = 2ull << 62, kValMask = (1ull << 62) - 1;
// look-back rounds without progress before a tile gives up and hands the
// input to the exact kernels (never expected: a safety valve that bounds the
// wait should a predecessor tile not be resident, see svm_fast.h tile order)
constexpr uint32_t kSpinLimit = 1u << 22;

// Diagnostic build only (-DDMLC_AMD_STAMPS, libdmlc_amd_stamps.so): thread 0
// of each tile records s_memtime at phase boundaries into g_stamps; the
// product build executes no stamp.
constexpr uint32_t kStampTiles = 1u << 17;
constexpr uint32_t kStampSlots = 20;  // per tile: 0 realtime start, 1.. phase ends, 15 look-back rounds
#if defined(DMLC_AMD_STAMPS) && defined(__HIPCC__)
__device__ uint64_t g_stamps[kStampTiles * kStampSlots];
#endif
#if defined(DMLC_AMD_STAMPS) && defined(__HIP_DEVICE_COMPILE__)
#define FAST_STAMP(k, i)                                                         \
  do {                                                                           \
    if (tid == 0 && (k) < kStampTiles) {                                         \
      __builtin_amdgcn_sched_barrier(0);                                         \
      g_stamps[(uint64_t)(k) * kStampSlots + (i)] =                                        \
          (i) == 0 ? __builtin_amdgcn_s_memrealtime() : __builtin_amdgcn_s_memtime(); \
      __builtin_amdgcn_sched_barrier(0);                                         \
    }                                                                            \
  } while (0)
#else
#define FAST_STAMP(k, i) \
  do {                   \
  } while (0)
#endif

// Byte classes by two 16-entry nibble tables (v_perm_b32 lookups): cls =
// LO[b & 15] & HI[b >> 4]; bits 0-2 digitchar (strtonum.h:70-72: 0-9, then
// + - ., then e E), bit 3 ':', bit 4 '\n' '\r', bits 5-6 ' ' '\t'
// (strtonum.h:37-39).  A zero class is a byte outside the grammar.
constexpr uint32_t kLoA = 0x01010121u, kLoB = 0x01010501u;  // LO[0..7]
constexpr uint32_t kLoC = 0x02184101u, kLoD = 0x00021200u;  // LO[8..15]
constexpr uint32_t kHiA = 0x09220050u, kHiB = 0x00040004u;  // HI[0..7]

struct Masks {
  uint64_t d, n, c;
  uint32_t bad;
  uint64_t g;   // table form: byte-1 plane (G digit for libsvm, outside-the-grammar for CSV)
  uint32_t hi;  // table form: a byte >= 0x80 among the 64 (its planes are not the table's)
};

// The class tables hold all 256 byte values (1 KiB of LDS per tile): a byte
// >= 0x80 has its own class (outside the grammar; CSV's junk), so the table
// body needs no per-byte range check.  (Round 4 tried 128 entries -- 512 B
// less LDS -- with the bytes >= 0x80 patched afterwards: the OR of the
// words that finds them cost the libfm kernel 7 spilled VGPRs, and the
// out-of-table reads leaked into neighbouring bytes' planes.)
constexpr int kClsEntries = 256;
DA_HD uint32_t cls_index(uint32_t b) { return b & 0xFFu; }
// bit i: byte i of the 64 at p (16-byte aligned) is >= 0x80 (rare: a slow loop)
DA_HD uint64_t hi_mask64(const uint8_t *p) {
  uint64_t m = 0;
  for (int i = 0; i < 64; ++i) m |= (uint64_t)(p[i] >> 7) << i;
  return m;
}
DA_HD uint32_t hi_nib4(uint32_t x) { return (((x >> 3) & 0x10101010u) * 0x01020408u) >> 28; }  // bytes >= 0x80

DA_HD uint32_t nib_d(uint32_t cls) {  // digitchar byte flags -> 4 bits
  return ((((cls & 0x07070707u) + 0x7F7F7F7Fu) & 0x80808080u) * 0x00204081u) >> 28;
}
DA_HD uint32_t nib_n(uint32_t cls) { return ((cls & 0x10101010u) * 0x01020408u) >> 28; }
DA_HD uint32_t nib_c(uint32_t cls) { return ((cls & 0x08080808u) * 0x02040810u) >> 28; }

DA_HD uint32_t classify4(uint32_t x) {
  const uint32_t lo = x & 0x0F0F0F0Fu, s = lo & 0x07070707u;
  const uint32_t a = perm_b32(kLoB, kLoA, s), b = perm_b32(kLoD, kLoC, s);
  const uint32_t m8 = ((lo >> 3) & 0x01010101u) * 0xFFu;
  const uint32_t lov = (b & m8) | (a & ~m8);
  const uint32_t hv = perm_b32(kHiB, kHiA, (x >> 4) & 0x07070707u);
  return lov & hv;
}

DA_HD void load16(const uint8_t *p, uint32_t w[4]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4 v = *reinterpret_cast<const uint4 *>(p);
  w[0] = v.x;
  w[1] = v.y;
  w[2] = v.z;
  w[3] = v.w;
#else
  memcpy(w, p, 16);
#endif
}

struct Nib {
  uint32_t d, n, c, bad, g, hi;
};
DA_HD Nib classify_dword(uint32_t x) {  // 4-bit masks of 4 bytes; bad: a byte outside the grammar
  const uint32_t cls = classify4(x);
  Nib r;
  r.d = nib_d(cls);
  r.n = nib_n(cls);
  r.c = nib_c(cls);
  r.bad = ((cls + 0x7F7F7F7Fu) & 0x80808080u) != 0x80808080u || (x & 0x80808080u);
  r.g = 0;
  r.hi = hi_nib4(x);
  return r;
}

// Masks of the 64 bytes at p (16-byte aligned).  Bytes past the end of the
// text are staged as blanks, so they are neutral here.
DA_HD Masks classify64(const uint8_t *p) {
  uint32_t dl = 0, dh = 0, nl = 0, nh = 0, cl = 0, ch = 0;
  uint32_t all = 0x80808080u, orv = 0;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w[4];
    load16(p + 16 * q, w);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int i = 4 * q + j;
      const uint32_t x = w[j];
      const uint32_t cls = classify4(x);
      all &= cls + 0x7F7F7F7Fu;
      orv |= x;
      const int sh = 4 * (i & 7);
      if (i < 8) {
        dl |= nib_d(cls) << sh;
        nl |= nib_n(cls) << sh;
        cl |= nib_c(cls) << sh;
      } else {
        dh |= nib_d(cls) << sh;
        nh |= nib_n(cls) << sh;
        ch |= nib_c(cls) << sh;
      }
    }
  }
  Masks m;
  m.d = dl | ((uint64_t)dh << 32);
  m.n = nl | ((uint64_t)nh << 32);
  m.c = cl | ((uint64_t)ch << 32);
  m.bad = ((all & 0x80808080u) != 0x80808080u) || (orv & 0x80808080u);
  m.g = 0;
  m.hi = (orv & 0x80808080u) != 0u;
  return m;
}

// ---- byte classes by table lookup (the VALU-cheap form on MI355X: one SDWA
// shift + one shift-or per byte, the lookup on the LDS pipe).  Entry planes:
// byte 0 D digitchar, 1 G digit, 2 N newline, 3 C colon; blanks are 0; a byte
// outside the grammar is G without D.  The letters of "qid:" (libsvm only,
// libsvm_parser.h:119-132) are N and C together, which no other byte is:
// svm_fast.h qid_clean turns them into blanks and the token's ':' into a
// qid marker (N and C) or flags them.
DA_HD uint32_t class_of(uint32_t b) {
  if (b - '0' < 10u) return 0x00000101u;
  if (b == '+' || b == '-' || b == '.' || b == 'e' || b == 'E') return 0x00000001u;
  if (b == '\n' || b == '\r') return 0x00010000u;
  if (b == ':') return 0x01000000u;
  if (b == ' ' || b == '\t') return 0u;
  if (b == 'q' || b == 'i' || b == 'd') return 0x01010000u;
  return 0x00000100u;
}

// Masks of the 64 bytes at p (16-byte aligned) through the class table.
DA_HD Masks classify64_lut(const uint8_t *p, const uint32_t *cls) {
  uint32_t acc[8];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    uint32_t w[4];
    load16(p + 16 * q, w);
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int b = 0; b < 4; ++b) {
        const int i = 16 * q + 4 * j + b;
        const uint32_t x = cls[cls_index((w[j] >> (8 * b)) & 0xFFu)];
        if ((i & 7) == 0) acc[i >> 3] = x;
        else acc[i >> 3] |= x << (i & 7);
      }
  }
  // byte p of acc[j] = plane p of bytes 8j..8j+7: gather plane bytes
  uint32_t pd[2], pg[2], pn[2], pc[2];
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const uint32_t t = perm_b32(acc[4 * h + 1], acc[4 * h], 0x05010400u);
    const uint32_t u = perm_b32(acc[4 * h + 3], acc[4 * h + 2], 0x05010400u);
    pd[h] = perm_b32(u, t, 0x05040100u);
    pg[h] = perm_b32(u, t, 0x07060302u);
    const uint32_t t2 = perm_b32(acc[4 * h + 1], acc[4 * h], 0x07030602u);
    const uint32_t u2 = perm_b32(acc[4 * h + 3], acc[4 * h + 2], 0x07030602u);
    pn[h] = perm_b32(u2, t2, 0x05040100u);
    pc[h] = perm_b32(u2, t2, 0x07060302u);
  }
  Masks m;
  m.d = pd[0] | ((uint64_t)pd[1] << 32);
  m.n = pn[0] | ((uint64_t)pn[1] << 32);
  m.c = pc[0] | ((uint64_t)pc[1] << 32);
  const uint64_t g = pg[0] | ((uint64_t)pg[1] << 32);
  m.g = g;
  m.hi = 0u;  // (the table classes bytes >= 0x80 itself)
  m.bad = (g & ~m.d) != 0;
  return m;
}

// 4 bytes (x) through the table: 4-bit masks (a byte >= 0x80: r.hi, planes
// cleared, bad; its table word is masked to the plane bits so that it cannot
// reach the other bytes' planes)
DA_HD Nib classify_dword_lut(uint32_t x, const uint32_t *cls) {
  uint32_t acc = 0;
#pragma unroll
  for (int b = 0; b < 4; ++b) acc |= (cls[cls_index((x >> (8 * b)) & 0xFFu)] & 0x01010101u) << b;
  const uint32_t h = hi_nib4(x), k = ~h & 0xFu;
  Nib r;
  r.d = acc & k;
  r.n = (acc >> 16) & k;
  r.c = (acc >> 24) & k;
  r.g = (acc >> 8) & k;
  r.bad = (r.g & ~r.d) != 0 || h != 0;
  r.hi = h;
  return r;
}

// One 16-byte unit (w, as staged) through the table: its four 16-bit plane
// pieces, bit b <-> byte b of the unit, as classify64_lut's planes have them.
struct Piece16 {
  uint32_t dg, nc;  // D | G << 16, N | C << 16
};
DA_HD Piece16 classify16_lut(const uint32_t w[4], const uint32_t *cls) {
  uint32_t acc[2];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int i = 4 * j + b;
      const uint32_t x = cls[cls_index((w[j] >> (8 * b)) & 0xFFu)];
      if ((i & 7) == 0) acc[i >> 3] = x;
      else acc[i >> 3] |= x << (i & 7);
    }
  // byte p of acc[h] = plane p of bytes 8h..8h+7
  Piece16 r;
  r.dg = perm_b32(acc[1], acc[0], 0x05010400u);
  r.nc = perm_b32(acc[1], acc[0], 0x07030602u);
  return r;
}

// The value of the lane d (1 or 2) away inside the caller's quad of lanes
// (lane ^ d; all four lanes active): a DPP quad_perm move on the device.
template <int D, class BK>
DA_HDF uint32_t quad_swap(uint32_t v, BK &bk) {
  static_assert(D == 1 || D == 2, "a neighbour inside the quad");
#if defined(__HIP_DEVICE_COMPILE__)
  (void)bk;  // quad_perm:[1,0,3,2] / [2,3,0,1]
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, D == 1 ? 0xB1 : 0x4E, 0xF, 0xF, false);
#else
  return bk.shfl(v, (bk.tid() & (kWave - 1)) ^ D);
#endif
}
// 4x4 exchange of the pieces of a quad: lanes 4q .. 4q+3 hold the pieces of
// the four quarters of one 64-byte segment; lane j of the quad returns plane
// j's 64-bit word of the segment (0 D, 1 G, 2 N, 3 C).  Two moves: 32-bit
// registers between lanes j and j ^ 2, 16-bit halves between j and j ^ 1.
template <class BK>
DA_HDF uint64_t quad_planes(const Piece16 &p, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
  const bool up = (lane & 2u) != 0u, odd = (lane & 1u) != 0u;
  const uint32_t got = quad_swap<2>(up ? p.dg : p.nc, bk), keep = up ? p.nc : p.dg;
  const uint32_t lo = up ? got : keep, hi = up ? keep : got;  // my register pair's, of lanes j & 1 and (j & 1) + 2
  const uint32_t h0 = perm_b32(hi, lo, 0x05040100u), h1 = perm_b32(hi, lo, 0x07060302u);  // low / high halves
  const uint32_t got2 = quad_swap<1>(odd ? h0 : h1, bk), keep2 = odd ? h1 : h0;
  const uint32_t ev = odd ? got2 : keep2, od = odd ? keep2 : got2;  // my plane's pieces of quarters 0, 2 / 1, 3
  return (uint64_t)perm_b32(od, ev, 0x05040100u) | ((uint64_t)perm_b32(od, ev, 0x07060302u) << 32);
}

struct AddU64 {
  DA_HD uint64_t operator()(uint64_t a, uint64_t b) const { return a + b; }
};

// ---- SWAR decoders on the first 16 bytes of a run (read from the staged LDS
// text with five aligned words).  Digits are located with byte-parallel masks
// and converted eight at a time (multiply-shift 8-digit conversion), then
// combined with exactly the reference's arithmetic.

DA_HD uint32_t funnel(uint32_t hi, uint32_t lo, uint32_t sft) {  // ((hi:lo) >> sft), sft < 32
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_alignbit(hi, lo, sft);
#else
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> sft);
#endif
}

DA_HD uint32_t nondigit8(uint64_t x) {  // bit i: byte i is not '0'..'9' (grammar bytes < 0x80)
  const uint64_t t = x ^ 0x3030303030303030ull;
  const uint64_t h = ((t + 0x7676767676767676ull) & 0x8080808080808080ull) >> 7;
  return (uint32_t)((h * 0x0102040810204080ull) >> 56);
}

DA_HD uint64_t parse8(uint64_t w) {  // 8 ASCII digits, first char in the low byte
  w = ((w & 0x0F0F0F0F0F0F0F0Full) * 2561ull) >> 8;
  w = ((w & 0x00FF00FF00FF00FFull) * 6553601ull) >> 16;
  return ((w & 0x0000FFFF0000FFFFull) * 42949672960001ull) >> 32;
}

struct W16 {
  uint64_t lo, hi;  // window bytes 0..7, 8..15
  DA_HD uint32_t byte(uint32_t p) const {
    return (uint32_t)((p < 8 ? lo >> (8 * p) : hi >> (8 * (p - 8))) & 0xFFu);
  }
  DA_HD uint64_t at(uint32_t a) const {  // bytes a .. a+7 (zero beyond the window)
    if (a == 0) return lo;
    if (a < 8) return (lo >> (8 * a)) | (hi << (64 - 8 * a));
    return a < 16 ? hi >> (8 * (a - 8)) : 0;
  }
  DA_HD uint64_t span8(uint32_t a, uint32_t len) const {  // value of len <= 8 digits at a
    if (len == 0) return 0;
    uint64_t w = at(a) << (8 * (8 - len));
    if (len < 8) w |= 0x3030303030303030ull >> (8 * len);
    return parse8(w);
  }
  DA_HD uint64_t span16(uint32_t a, uint32_t len) const {  // len <= 16
    return len <= 8 ? span8(a, len) : span8(a, len - 8) * 100000000ull + span8(a + len - 8, 8);
  }
  DA_HD uint32_t digits() const { return ~(nondigit8(lo) | (nondigit8(hi) << 8)) & 0xFFFFu; }
};

DA_HD uint32_t run_len(uint32_t dm, uint32_t a) {  // consecutive digits from byte a
  return a >= 16 ? 0 : (uint32_t)ctz32(~(dm >> a));
}

DA_HD double pow10_exact(uint32_t k) {  // 10^k as a double, exact for k <= 22
  double p = 1.0;
  if (k & 1u) p *= 10.0;
  if (k & 2u) p *= 100.0;
  if (k & 4u) p *= 1e4;
  if (k & 8u) p *= 1e8;
  if (k & 16u) p *= 1e16;
  return p;
}

// ParseFloat<float> (strtonum.h:95-264) restated for a run of the uniform
// grammar -- inf / nan / the 'f' suffix need letters outside it -- with the
// reference's operations: u64 integer part, f32 conversion, one f64 division
// of the (<= 19-digit) fraction, f32 add, f32 exponent scaling.
// *ok = false when the number may continue past the window (caller falls back).
DA_HD float wfloat(const W16 &w, bool *ok) {
  const uint32_t dm = w.digits();
  const uint32_t b0 = w.byte(0);
  const bool sign = b0 != '-';
  const uint32_t s = (b0 == '-' || b0 == '+') ? 1u : 0u;
  const uint32_t il = run_len(dm, s);
  uint32_t p = s + il;
  *ok = false;
  if (p >= 16) return 0.f;
  float value = (float)w.span16(s, il);
  uint32_t c = w.byte(p);
  if (c == '.') {
    const uint32_t fs = p + 1;
    const uint32_t fl = run_len(dm, fs);
    p = fs + fl;
    if (p >= 16) return 0.f;
    value += (float)((double)w.span16(fs, fl) / pow10_exact(fl));
    c = w.byte(p);
  }
  if (c == 'e' || c == 'E') {
    bool frac = false;
    float scale = 1.0f;
    if (++p >= 16) return 0.f;
    c = w.byte(p);
    if (c == '-' || c == '+') {
      frac = c == '-';
      if (++p >= 16) return 0.f;
      c = w.byte(p);
    }
    uint32_t expon = 0;
    for (; is_digit(c); c = w.byte(p)) {
      expon = expon * 10u + (c - '0');
      if (++p >= 16) return 0.f;
    }
    if (expon > 38u) expon = 38u;
    const float kMaxSig = (float)3.402823466, kMaxSigNeg = (float)1.175494351;
    if (expon == 38u && ((!frac && value > kMaxSig) || (frac && value < kMaxSigNeg)))
      value = frac ? kMaxSigNeg : kMaxSig;
    while (expon >= 8u) {
      scale *= 1E8f;
      expon -= 8u;
    }
    while (expon > 0u) {
      scale *= 10.0f;
      expon -= 1u;
    }
    value = frac ? (value / scale) : (value * scale);
  }
  *ok = true;
  return sign ? value : -value;
}

// ParseUnsignedInt (strtonum.h:392-428) on a run (no leading blanks there):
// false on a leading '-' (the reference's fatal CHECK).  Up to 16 digits the
// exact value truncated to the index width equals the reference's wrapping
// accumulation.
DA_HD bool wuint(const W16 &w, bool wide, uint64_t *out, bool *ok) {
  const uint32_t b0 = w.byte(0);
  *ok = true;
  if (b0 == '-') return false;
  const uint32_t s = b0 == '+' ? 1u : 0u;
  const uint32_t il = run_len(w.digits(), s);
  if (s + il >= 16) {
    *ok = false;
    return true;
  }
  const uint64_t v = w.span16(s, il);
  *out = wide ? v : (uint64_t)(uint32_t)v;
  return true;
}

// ---- 32-bit decoders (MI355X: v_dot4_u32_u8, 32-bit mul and perm are full
// rate; 64-bit multiplies and the f64 divide sequence are not)
struct DecTables {
  double p10[16], i10[16];  // 10^k and RN(10^-k)
  uint64_t hib[9];          // 0x0F in bytes >= k of 8 (k <= 8): the fraction's byte masks
};
// The tables as compile-time constants (constant evaluation divides with
// IEEE round-to-nearest, so i10[k] is the correctly rounded 10^-k): what
// init_dec_tables must produce, bit for bit (tests/emu/chunk_guess_check.cpp,
// the decoders' goldens on the device).
constexpr DecTables make_dec_tables() {
  DecTables t{};
  double p = 1.0;
  for (int k = 0; k < 16; ++k) {
    t.p10[k] = p;
    t.i10[k] = 1.0 / p;
    p *= 10.0;
  }
  for (int k = 0; k <= 8; ++k) {
    uint64_t m = 0;
    for (int b = k; b < 8; ++b) m |= 0x0Full << (8 * b);
    t.hib[k] = m;
  }
  return t;
}
constexpr DecTables kDecTables = make_dec_tables();
// Threads first .. first + 24 of the block fill the tile's copy in LDS, each
// entry computed in registers: 10^t is an exact product of 10, 100, 1e4 and
// 1e8 (t < 16: every partial product is below 2^53), 10^-t one IEEE f64
// divide.  (Copied from kDecTables, each lane's global load was followed at
// once by a full vmcnt(0) wait -- one more dependent trip to memory on the
// tile prologue's path, which also drained every load issued before it.)
// The single-pass tiles give the job to their last wave (first = its first
// thread): wave 0 has the chunk list to make before the stage barrier.
template <class BK>
DA_HDF void init_dec_tables(DecTables &tb, BK &bk, int first = 0) {
  const int t = bk.tid() - first;
  if (t >= 0 && t < 16) {
    const double p = pow10_exact((uint32_t)t);
    tb.p10[t] = p;
    tb.i10[t] = 1.0 / p;
  } else if (t >= 16 && t < 25) {
    const uint32_t k = (uint32_t)t - 16u;
    tb.hib[k] = k >= 8u ? 0ull : 0x0F0F0F0F0F0F0F0Full << (8u * k);
  }
}
DA_HD uint32_t udot4(uint32_t a, uint32_t b, uint32_t c) {  // sum of the 4 byte products + c
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_udot4(a, b, c, false);
#else
  for (int i = 0; i < 4; ++i) c += ((a >> (8 * i)) & 0xFFu) * ((b >> (8 * i)) & 0xFFu);
  return c;
#endif
}
// acc * 10^4 + the 4-digit value of the nibbles d (byte 0 most significant)
DA_HD uint32_t dig4(uint32_t d, uint32_t acc) {
  const uint32_t t = udot4(d, 0x0000010Au, acc * 100u);  // acc*100 + 10 d0 + d1
  return udot4(d, 0x010A0000u, t * 100u);                // t*100 + 10 d2 + d3
}
DA_HD uint32_t nd4(uint32_t x) {  // 4 bits: byte i is not '0'..'9' (bytes < 0x80)
  return udot4((((x ^ 0x30303030u) + 0x76767676u) >> 7) & 0x01010101u, 0x08040201u, 0u);
}
DA_HD uint32_t byte_of(const uint32_t w[4], uint32_t p) {  // window byte p < 16 (one v_perm)
  // (the four words as values: a select between array elements compiled to
  // a dynamically indexed private array, i.e. scratch memory)
  const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3];
  const bool h = (p & 8u) != 0u;
  return perm_b32(h ? w3 : w1, h ? w2 : w0, (p & 7u) | 0x0C0C0C00u);
}
DA_HD uint64_t low_bytes(uint32_t k) {  // mask of the low k bytes, k <= 8
  return k >= 8 ? ~0ull : ((1ull << (8u * k)) - 1ull);
}
// value of the L <= 8 decimal digits at window bytes s .. s+L-1 (s <= 1): the
// 8 bytes from s shifted up so the digits end at byte 7 -- the bytes after
// them fall off the top, zeros enter below -- then 4 + 4 digits by dot4 (no
// division by 10^(8-L), no table)
DA_HD uint32_t digits_ra(const uint32_t w[4], uint32_t s, uint32_t L) {
  const uint32_t sh = 8u * s;
  const uint64_t x = ((uint64_t)funnel(w[2], w[1], sh) << 32) | funnel(w[1], w[0], sh);
  const uint64_t y = L ? x << (64u - 8u * L) : 0ull;
  return dig4((uint32_t)(y >> 32) & 0x0F0F0F0Fu, dig4((uint32_t)y & 0x0F0F0F0Fu, 0u));
}

// ParseFloat<float> (strtonum.h:95-264) on a run of the uniform grammar,
// 32-bit form: integer part (<= 8 digits) right-aligned by a shift and
// converted by dot4 (digits_ra); the fraction digits [fs, pe) -- the window
// shifted up so byte pe - 1 lands on byte 15, the bytes below the fraction
// cleared -- give val2 exactly (< 10^15), and val2 / 10^fl, the reference's
// (double)val2/(double)pow10, is rounded by a Markstein quotient (one
// multiply, two FMAs, tabulated reciprocal).  The reference's arithmetic is
// kept: integer part -> f32, f64 fraction -> f32, f32 add.  *ok = false:
// exponent, long parts or a number that may continue past the window (caller
// falls back to the byte decoder).
// M: bit i set when window byte i is not '0'..'9' (16 bits)
// Straight-line (no early return: a decoder in a loop of the tile kernels
// must not split the wave's exec mask); the value is meaningless when *ok is
// false.
DA_HD float wfloat32m(const uint32_t w[4], uint32_t M, const DecTables &tb, bool *ok) {
  const uint32_t b0 = w[0] & 0xFFu;
  const bool neg = b0 == '-';
  const uint32_t sg = (neg || b0 == '+') ? 1u : 0u;
  const uint32_t p = (uint32_t)ctz32((M & ~sg) | 0x10000u);  // 0..16
  const uint32_t pc = p & 15u;
  const uint32_t c = byte_of(w, pc);
  const bool dot = c == '.';
  const uint32_t fs = pc + 1u;  // 1..16
  const uint32_t pd = (uint32_t)ctz32((M & ~((2u << pc) - 1u)) | 0x10000u);
  const uint32_t cd = byte_of(w, pd & 15u);
  const uint32_t pe = dot ? pd : pc;
  const uint32_t ce = dot ? cd : c;
  const uint32_t il = p - sg;
  *ok = p < 16u && pe < 16u && (ce | 0x20u) != 'e' && il <= 8u;
  const uint32_t iv = digits_ra(w, sg, il < 8u ? il : 8u);
  // fraction bytes [fs, pe) (empty without a '.', pe < fs): tabulated byte
  // masks of each 8-byte half
  const uint32_t pk = pe < 16u ? pe : 16u;
  const uint32_t fs8 = fs < 8u ? fs : 8u, pe8 = pk < 8u ? pk : 8u;
  const uint32_t fsh = fs > 8u ? fs - 8u : 0u, peh = pk > 8u ? pk - 8u : 0u;
  const uint64_t flo = ((uint64_t)w[1] << 32 | w[0]) & tb.hib[fs8] & ~tb.hib[pe8];
  const uint64_t fhi = ((uint64_t)w[3] << 32 | w[2]) & tb.hib[fsh] & ~tb.hib[peh];
  const uint32_t fh = dig4((uint32_t)(flo >> 32), dig4((uint32_t)flo, 0u));
  const uint32_t fo = dig4((uint32_t)(fhi >> 32), dig4((uint32_t)fhi, 0u));
  const double v = __builtin_fma((double)fh, 1e8, (double)fo);  // exact: < 10^15
  const uint32_t e = 16u - fs;                                  // 0..15
  const double r = tb.i10[e], t = v * r;
  const double q = __builtin_fma(r, __builtin_fma(-t, tb.p10[e], v), t);
  const float value = (float)iv + (float)q;
  return neg ? -value : value;
}
DA_HD float wfloat32(const uint32_t w[4], const DecTables &tb, bool *ok) {
  return wfloat32m(w, nd4(w[0]) | (nd4(w[1]) << 4) | (nd4(w[2]) << 8) | (nd4(w[3]) << 12), tb, ok);
}

// ParseUnsignedInt (strtonum.h:392-428): [+] then up to 8 digits.  Returns
// false on a leading '-' (the reference's fatal CHECK); *ok = false when the
// digits may not fit the form (caller falls back).
// M: bit i set when window byte i is not '0'..'9' (bits 0-11 used)
DA_HD bool wuint32m(const uint32_t w[4], uint32_t M, const DecTables &tb, uint64_t *out, bool *ok) {
  (void)tb;
  const uint32_t b0 = w[0] & 0xFFu;
  const uint32_t s = b0 == '+' ? 1u : 0u;
  M = (M & 0xFFFu) | 0x1000u;
  const uint32_t L = (uint32_t)ctz32(M & ~s) - s;
  *ok = L <= 8u;  // branch-free, as wfloat32m
  *out = digits_ra(w, s, L < 8u ? L : 8u);
  return b0 != '-';
}
DA_HD bool wuint32(const uint32_t w[4], const DecTables &tb, uint64_t *out, bool *ok) {
  return wuint32m(w, nd4(w[0]) | (nd4(w[1]) << 4) | (nd4(w[2]) << 8), tb, out, ok);
}

struct GSrc {  // text bytes; NUL at or beyond the chunk end (as Src), global memory
  const uint8_t *g;
  uint64_t lim;
  DA_HD uint32_t operator()(uint64_t p) const { return p < lim ? (uint32_t)g[p] : 0u; }
};

// the 16 bytes at absolute position q (staged in LDS at `text`, which holds
// position tlo - kPre at index 0; q < tile end) as a window
DA_HD W16 win_at(const uint8_t *text, uint64_t tlo, uint64_t q) {
  const uint32_t off = (uint32_t)(q - tlo) + kPre;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(text + (off & ~3u));
  const uint32_t sft = (off & 3u) * 8u;
  const uint32_t x0 = w[0], x1 = w[1], x2 = w[2], x3 = w[3], x4 = w[4];
  W16 r;
  r.lo = funnel(x1, x0, sft) | ((uint64_t)funnel(x2, x1, sft) << 32);
  r.hi = funnel(x3, x2, sft) | ((uint64_t)funnel(x4, x3, sft) << 32);
  return r;
}

// the same at tile offset o (position tlo + o)
DA_HD W16 win_at_o(const uint8_t *text, uint32_t o) {
  const uint32_t off = o + kPre;
  const uint32_t *w = reinterpret_cast<const uint32_t *>(text + (off & ~3u));
  const uint32_t sft = (off & 3u) * 8u;
  const uint32_t x0 = w[0], x1 = w[1], x2 = w[2], x3 = w[3], x4 = w[4];
  W16 r;
  r.lo = funnel(x1, x0, sft) | ((uint64_t)funnel(x2, x1, sft) << 32);
  r.hi = funnel(x3, x2, sft) | ((uint64_t)funnel(x4, x3, sft) << 32);
  return r;
}

// ---- per-tile state every fast kernel keeps in LDS
struct TileCommon {
  alignas(16) uint8_t text[kStage];  // position p <-> text[p - tlo + kPre]
  uint64_t csl[kMaxCs + 1];           // chunk starts in [tlo, thi]
  uint64_t cfloor, cnext, base[4];    // last chunk start <= tlo, first beyond the list, output bases
  uint32_t ncs, c_first, toomany, bad;
};

// Wave 0 (all 64 lanes): the chunk starts touching [tlo, thi].  The chunk of
// tlo is found by a 64-ary search -- one round of 64 independent loads per
// factor of 64 chunks, instead of a dependent binary-search chain per tile
// (9 loads at 257 chunks, the longest latency of the tile prologue) -- and the
// list comes from one more window load: csl = cs[c_first ..] inside [tlo, thi]
// (excluding cs[nchunk]), cnext = the entry after the list (cs[nchunk] == n).
//
// In two halves: chunk_list_begin runs the search rounds and issues the window
// load, chunk_list_end consumes it.  The tile prologues first try the one
// window a guess gives them (chunk_guess_begin / chunk_guess_end below) and
// come here when it misses.

// (the staged range in 16-byte units and load rounds: stage_issue below)
constexpr int kStageUnits = kStage / 16;
constexpr int kStageRounds = (kStageUnits + kFThreads - 1) / kFThreads;
static_assert(kStage % 16 == 0, "staged range is whole 16-byte units");
struct ChunkProbe {
  uint64_t lo, cnt, v;
};
template <class BK>
DA_HDF ChunkProbe chunk_list_begin(const uint64_t *cs, int nchunk, uint64_t tlo, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
  const uint64_t kBig = ~0ull;
  // invariant: cs[lo] <= tlo, the answer (last i < nchunk with cs[i] <= tlo) lies in [lo, lo + cnt)
  uint64_t lo = 0, cnt = (uint64_t)nchunk;
  while (cnt > (uint64_t)kWave) {
    const uint64_t S = (cnt + kWave - 1) / kWave;
    const uint64_t i = lo + lane * S;
    const uint64_t v = (lane * S < cnt) ? cs[i] : kBig;
    const uint64_t m = bk.ballot(v <= tlo);
    const uint64_t j = 63 - clz64(m);  // lane 0 always holds (cs[lo] <= tlo)
    const uint64_t nlo = lo + j * S;
    cnt = mn<uint64_t>(S, lo + cnt - nlo);
    lo = nlo;
  }
  // window cs[lo .. lo + 64) (entries past cs[nchunk] read as "beyond")
  ChunkProbe p;
  p.lo = lo;
  p.cnt = cnt;
  p.v = lo + lane <= (uint64_t)nchunk ? cs[lo + lane] : kBig;
  return p;
}
// The list of the window v = cs[lo + lane] (beyond cs[nchunk]: kBig), where
// cs[c0] is the chunk of tlo and c0 - lo <= kWave - kMaxCs - 2.  fits_only:
// write nothing and return false when the tile holds more than kMaxCs starts
// (toomany: the caller takes the search, whose window decides cnext then).
template <class BK>
DA_HDF bool chunk_list_write(int nchunk, uint64_t tlo, uint64_t thi, uint64_t lo, uint64_t v, uint64_t c0,
                             bool fits_only, TileCommon &c, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
  const uint64_t kBig = ~0ull;
  const uint64_t idx = lo + lane;
  const uint64_t vf = bk.shfl(v, (int)(c0 - lo));  // cs[c0]
  const uint32_t first = (uint32_t)(c0 - lo) + (vf < tlo ? 1u : 0u);  // lane of c_first
  const uint64_t lm = bk.ballot(lane >= first && idx < (uint64_t)nchunk && v <= thi);
  const uint32_t m_all = (uint32_t)popc64(lm);
  const uint32_t ln = first + m_all;                                 // lane of cnext
  const bool over = m_all > (uint32_t)kMaxCs || ln >= (uint32_t)kWave;
  if (fits_only && over) return false;  // wave-uniform
  const uint64_t vn = bk.shfl(v, (int)(ln < (uint32_t)kWave ? ln : 0u));
  if (lane >= first && lane - first < (uint32_t)kMaxCs && ((lm >> lane) & 1u)) c.csl[lane - first] = v;
  if (lane == 0) {
    c.cfloor = vf;
    c.c_first = (uint32_t)(lo + first);
    c.ncs = over ? (uint32_t)kMaxCs : m_all;
    c.cnext = ln < (uint32_t)kWave ? vn : kBig;
    c.toomany = over;
    c.bad = 0;
  }
  return true;
}
template <class BK>
DA_HDF void chunk_list_end(const uint64_t *cs, int nchunk, uint64_t tlo, uint64_t thi, const ChunkProbe &p,
                           TileCommon &c, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
  const uint64_t kBig = ~0ull;
  uint64_t lo = p.lo, v = p.v;
  const uint64_t cnt = p.cnt;
  uint64_t m = bk.ballot(lane < cnt && v <= tlo);
  const uint64_t c0 = lo + (63 - clz64(m));
  if (c0 - lo > (uint64_t)(kWave - kMaxCs - 2)) {  // the list may run past the window: reload at c0
    lo = c0;
    v = lo + lane <= (uint64_t)nchunk ? cs[lo + lane] : kBig;
  }
  (void)chunk_list_write(nchunk, tlo, thi, lo, v, c0, false, c, bk);
}
// The search form: one dependent trip to memory per factor of 64 chunks, one
// for the window, one more when the list may run past it.
template <class BK>
DA_HDF void chunk_list(const uint64_t *cs, int nchunk, uint64_t tlo, uint64_t thi, TileCommon &c,
                       BK &bk) {
  const ChunkProbe p = chunk_list_begin(cs, nchunk, tlo, bk);
  chunk_list_end(cs, nchunk, tlo, thi, p, c, bk);
}

// The one-trip form the tile prologues use.  Unit starts are near-uniform in
// real use -- InputSplit cuts equal buffers after their last newline, FillData
// splits each evenly -- so the unit of tlo is close to tlo * nchunk / n.
// chunk_guess_begin loads the one window of cs that puts that estimate
// kGuessBack lanes in (the whole table when it fits a window); the caller
// issues it BEFORE the tile's text loads, so that the wait for it is a
// partial one (vector-memory returns count in order) with the text still in
// flight.  chunk_guess_end makes the list from it when the window brackets
// tlo low enough for the list to follow in it (chunk_list_end's condition)
// and the tile holds at most kMaxCs starts; otherwise -- units far from
// uniform, a found unit in the window's last lanes, toomany -- the search
// above runs, so TileCommon is the search's for every input.
//
// The partial wait is spelled out.  The compiler places s_waitcnt from the
// fewest loads any path puts after the one it waits for, and the paths that
// stage no text (a tile at an end of the text) or skip a lane-guarded load
// put fewer after the window load than wave 0 of an interior tile does: left
// to it, the wait is vmcnt(0) -- the whole text fetch.  So on the device the
// window load is an asm statement the compiler does not count, and
// chunk_guess_end waits for it by hand: vmcnt(kStageRounds) when stage_issue
// has put the text loads after it (text_in_flight: wave 0 executes each of
// the kStageRounds load instructions -- its thread 0 owns a unit of every
// round), vmcnt(0) otherwise.  More vector-memory instructions in between
// than counted only make the wait stricter; the "memory" clobbers keep the
// text loads between the two statements.
constexpr int kGuessBack = (kWave - kMaxCs - 2) / 2;
static_assert(kStageUnits > (kStageRounds - 1) * kFThreads, "thread 0 loads a unit in every stage round");
template <class BK>
DA_HDF ChunkProbe chunk_guess_begin(const uint64_t *cs, int nchunk, uint64_t n, uint64_t tlo, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
  uint64_t lo = 0;
  if (nchunk >= kWave) {  // (else cs[0 .. nchunk] is one window)
    // a float estimate: off by a 2^-22 of nchunk at most, far inside the window
    const float g = (float)tlo * ((float)nchunk / (float)n);  // tlo < n: 0 <= g < 1.000001 nchunk
    const uint32_t gi = mn<uint32_t>((uint32_t)g, (uint32_t)nchunk - 1u);
    lo = gi > (uint32_t)kGuessBack ? gi - (uint32_t)kGuessBack : 0u;
  }
  ChunkProbe p;
  p.lo = lo;
  p.cnt = (uint64_t)kWave;
  // (lanes past cs[nchunk] load it again; chunk_guess_end reads them as "beyond")
  const uint64_t *src = cs + mn<uint64_t>(lo + lane, (uint64_t)nchunk);
#if defined(__HIP_DEVICE_COMPILE__)
  asm volatile("global_load_dwordx2 %0, %1, off" : "=v"(p.v) : "v"(src) : "memory");
#else
  p.v = *src;
#endif
  return p;
}
template <class BK>
DA_HDF void chunk_guess_end(const uint64_t *cs, int nchunk, uint64_t tlo, uint64_t thi, ChunkProbe &p,
                            bool text_in_flight, TileCommon &c, BK &bk) {
  const uint32_t lane = (uint32_t)bk.tid();
#if defined(__HIP_DEVICE_COMPILE__)
  // One statement for both waits, on p.v itself: until it has run, p.v is a
  // register still being loaded that the compiler takes for written, so
  // nothing may read or copy it first.  (Two statements, one per branch of an
  // `if`, made the compiler join their results -- with a copy of p.v ahead of
  // the wait on one side.)
  asm volatile(
      "s_cmp_eq_u32 %1, 0\n\t"
      "s_cbranch_scc1 1f\n\t"
      "s_waitcnt vmcnt(%2)\n\t"
      "s_branch 2f\n"
      "1:\n\t"
      "s_waitcnt vmcnt(0)\n"
      "2:"
      : "+v"(p.v)
      : "s"(__builtin_amdgcn_readfirstlane((uint32_t)text_in_flight)), "n"(kStageRounds)  // (wave-uniform)
      : "scc", "memory");
#else
  (void)text_in_flight;
#endif
  uint64_t v = p.v;
  if (p.lo + lane > (uint64_t)nchunk) v = ~0ull;
  // lanes at or before the unit of tlo: a prefix of the window (cs ascends)
  const uint64_t m = bk.ballot(p.lo + lane < (uint64_t)nchunk && v <= tlo);
  const uint32_t top = 63u - (uint32_t)clz64(m | 1u);
  bool done = false;
  if ((m & 1u) && top <= (uint32_t)(kWave - kMaxCs - 2))  // wave-uniform
    done = chunk_list_write(nchunk, tlo, thi, p.lo, v, p.lo + top, true, c, bk);
  if (!done) chunk_list(cs, nchunk, tlo, thi, c, bk);
}

// All threads: stage [tlo - kPre, tlo + kTile + kPost) into LDS with 16-byte
// loads; bytes past the end of the text become blanks (neutral to every
// classifier, never decoded).  The caller synchronises.
template <class BK>
DA_HDF void stage(const uint8_t *text, uint64_t n, uint64_t tlo, TileCommon &c, BK &bk) {
  const uint64_t s0 = tlo >= (uint64_t)kPre ? tlo - kPre : 0;
  const uint64_t s1 = tlo + kTile + kPost;
  uint8_t *dst = c.text + (s0 + kPre - tlo);
  const uint64_t nunits = (s1 - s0) >> 4;
  for (uint64_t u = bk.tid(); u < nunits; u += kFThreads) {
    const uint64_t g = s0 + (u << 4);
    uint32_t w[4];
    if (g + 16 <= n) {
      load16(text + g, w);
    } else {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        uint32_t x = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const uint64_t pos = g + 4 * q + b;
          x |= (uint32_t)(pos < n ? text[pos] : (uint8_t)' ') << (8 * b);
        }
        w[q] = x;
      }
    }
    memcpy(dst + (u << 4), w, 16);
  }
}

// The same staging split in two so every load of the tile is in flight at
// once: stage_issue loads each thread's 16-byte units into registers (all
// kStageRounds loads before any wait), stage_commit writes them to LDS.  The
// caller puts the tile's other prologue work (chunk list, tables) between the
// two, so its latency overlaps the loads'.  (A single loop of load -> LDS
// store waited for each load in turn: 5 HBM round trips per tile, ~14k cycles
// of a ~57k-cycle tile.)  Tiles whose staged range leaves the text take the
// byte-wise path of stage() at commit time.
struct StageRegs {
  uint32_t w[kStageRounds][4];
  bool interior;
};
// kEveryLane: every lane executes every round's load, the lanes past the
// staged range loading its last unit again (never stored).  A consumer that
// takes the rounds one by one as they land (svm_fast.h front_half) needs it:
// the compiler sizes the wait for round i from the fewest loads any path puts
// after it, and a lane-guarded load is one a path may skip -- with the guards,
// the wait for round 0 was vmcnt(0), the whole tile's text.
template <bool kEveryLane = false, class BK>
DA_HDF void stage_issue(const uint8_t *text, uint64_t n, uint64_t tlo, StageRegs &r, BK &bk) {
  // (kEveryLane: the caller has established that the tile is interior)
  r.interior = kEveryLane || (tlo >= (uint64_t)kPre && tlo + kTile + kPost <= n);
  if (!r.interior) return;
  const uint8_t *src = text + (tlo - kPre);
  const int t = bk.tid();
#pragma unroll
  for (int i = 0; i < kStageRounds; ++i) {
    const int u = t + i * kFThreads;
    if (kEveryLane) {
      load16(src + 16 * mn<int>(u, kStageUnits - 1), r.w[i]);
      sched_fence();  // in the rounds' order (the scheduler put round 0 behind rounds 1 to 3)
    } else if (u < kStageUnits) {
      load16(src + 16 * u, r.w[i]);
    }
  }
}
template <class BK>
DA_HDF void stage_commit(const uint8_t *text, uint64_t n, uint64_t tlo, const StageRegs &r, TileCommon &c,
                         BK &bk) {
  if (!r.interior) {
    stage(text, n, tlo, c, bk);
    return;
  }
  const int t = bk.tid();
#pragma unroll
  for (int i = 0; i < kStageRounds; ++i) {
    const int u = t + i * kFThreads;
    if (u < kStageUnits) memcpy(c.text + 16 * u, r.w[i], 16);
  }
}

// ---- decoupled look-back records.  Two arrays: st[ntiles], one 8-byte
// status word per tile -- bits 62-63 state (1 aggregate, 2 inclusive) | the
// tile's four counts packed 15 bits each (a 16 KiB tile holds < 2^15 of
// anything) -- and incl[ntiles][4], the inclusive prefix per counter, written
// and drained (vmcnt(0)) before the status turns inclusive.  The status words
// of consecutive tiles share cache lines: one poll instruction of a wave reads
// 64 predecessors' words (512 contiguous bytes, 4 lines), where a record of a
// line per tile cost a line per predecessor.  (kLbPer > 1 polls more
// predecessors per round; measured slower at 4.)
constexpr uint64_t kSAgg = 1ull << 62, kSIncl = 2ull << 62;
#ifndef FSVM_LB_PER
#define FSVM_LB_PER 1
#endif
constexpr int kLbPer = FSVM_LB_PER;  // predecessors polled per lane per round
DA_HD uint64_t pack4(const uint32_t c[4]) {
  return (uint64_t)c[0] | ((uint64_t)c[1] << 15) | ((uint64_t)c[2] << 30) | ((uint64_t)c[3] << 45);
}

// Inclusive prefixes are tagged words: incl[k][f] = kMark | value, each an
// untorn 8-byte granule that the launch's memset left 0, so a reader takes
// a tile's inclusive prefix as soon as all four of its words carry the mark
// -- no drain between the prefix and a status flag, and the reader polls a
// predecessor's status word and prefix words in the same round trip.
constexpr uint64_t kMark = 1ull << 63;

// Lane 0: publish this tile's aggregate (tile 0 publishes its inclusive).
// kf / seed: a launch that resumes at tile kf (svm_lean.h) -- tile kf is the
// first, its exclusive prefix is seed[4] (tagged inclusive words of the
// launch before: the mark is dropped).
DA_HD void publish_aggregate(uint64_t *lb, uint32_t ntiles, uint32_t k, const uint32_t cnt[4], uint32_t kf = 0,
                             const uint64_t *seed = nullptr) {
  uint64_t *st = lb, *incl = lb + ntiles;
  if (k == kf) {
    for (int i = 0; i < 4; ++i) store_agent_u64(incl + (uint64_t)k * 4 + i, kMark | ((seed ? seed[i] & ~kMark : 0) + cnt[i]));
  } else {
    store_agent_u64(st + k, kSAgg | pack4(cnt));
  }
}

// Wave 0: decoupled look-back.  Lane l polls predecessor j-1-l: its status
// word (512 contiguous bytes per wave) and its four prefix words; a round
// consumes predecessors up to the nearest one with a complete inclusive
// prefix and stops before the nearest unpublished one.  cnt = this tile's
// counts (wave uniform).  Ends with c.base[0..3] = exclusive prefixes and
// publishes the inclusive prefix.  Returns the number of rounds.  The caller
// synchronises.
template <class BK>
DA_HDF uint32_t look_back(uint64_t *lb, uint32_t ntiles, uint32_t k, const uint32_t cnt[4], uint32_t *gate,
                          TileCommon &c, BK &bk, uint32_t kf = 0, const uint64_t *seed = nullptr) {
  const uint32_t lane = bk.tid();
  uint64_t *st = lb, *incl = lb + ntiles;
  uint64_t j = k;
  uint32_t spins = 0, rounds = 0;
  uint64_t acc[4] = {0, 0, 0, 0};
  if (k == kf && seed)
    for (int f = 0; f < 4; ++f) acc[f] = seed[f] & ~kMark;
  bool done = k == kf;  // (a resumed launch: tile kf published its inclusive prefix, svm_lean.h)
  while (!done) {
    ++rounds;
    uint64_t s = 0, w[4] = {kMark, kMark, kMark, kMark};  // before tile 0: an inclusive 0
    if (lane < j) {
      const uint64_t p = j - 1 - lane;
      s = load_agent_u64(st + p);
#pragma unroll
      for (int f = 0; f < 4; ++f) w[f] = load_agent_u64(incl + p * 4 + f);
    }
    const bool inc = (w[0] & w[1] & w[2] & w[3] & kMark) != 0;
    const uint64_t mi = bk.ballot(inc), mz = bk.ballot(!inc && (s >> 62) == 0);
    uint64_t D = kWave;  // predecessors that contribute their aggregates
    bool stop_incl = false;
    if (mz | mi) {
      D = (uint64_t)ctz64(mz | mi);
      stop_incl = (mi >> D) & 1u;
    }
    uint32_t part[4] = {0, 0, 0, 0};
    if (lane < D) {
#pragma unroll
      for (int f = 0; f < 4; ++f) part[f] = (uint32_t)((s >> (15 * f)) & 0x7FFFu);
    }
#pragma unroll
    for (int f = 0; f < 4; ++f) acc[f] += bk.wave_sum(part[f]);
    if (stop_incl) {
      done = true;
#pragma unroll
      for (int f = 0; f < 4; ++f) acc[f] += bk.shfl(w[f] & ~kMark, (int)D);
    } else {
      j -= D;
      if (D == 0) {
        if (++spins > kSpinLimit) {  // never expected: hand the input to the exact path
          if (lane == 0) atomic_or_u32(gate, 2u);
          done = true;
        }
        spin_pause();
      }
    }
  }
  if (lane < 4) {
    const uint64_t v = acc[lane == 0 ? 0 : lane == 1 ? 1 : lane == 2 ? 2 : 3];
    c.base[lane] = v;
    if (k > kf) store_agent_u64(incl + (uint64_t)k * 4 + lane, kMark | (v + cnt[lane == 0 ? 0 : lane == 1 ? 1 : lane == 2 ? 2 : 3]));
  }
  return rounds;
}
// words of look-back state per tile the launch must zero (status + prefix)
constexpr uint64_t kLbWords = kFastLbWords;  // args.h: the launcher sizes the workspace by it

}  // namespace fast
}  // namespace dmlc_amd
