// TEST INFRASTRUCTURE ONLY: the number catalogue of tests/numcat.py through
// the window decoders (fast_common.h wfloat32 / wuint32, csv_fast.h wint64m)
// and the exact kernels' front ends (exact_dec.h value_at / csv_value_at /
// index_at), host-compiled.  Each input line is "<kind> <tag> <string>":
// kind f (float) / i (index) / n (CSV integer), tag w (the window form must
// accept) / b (it must decline, or the kernels never ask it).  Fails when a
// decoder's *ok differs from the tag or a value differs from the byte decoder
// of decode.h.  usage: numcat_check <file>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "fast_common.h"
#include "csv_fast.h"
#include "csv_core.h"
#include "libsvm_core.h"

using namespace dmlc_amd;
using namespace dmlc_amd::fast;

struct Blk {
  int t;
  int tid() const { return t; }
};

static bool all_of(const std::string &s, const char *set) {
  for (char c : s)
    if (!strchr(set, c)) return false;
  return !s.empty();
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  FILE *f = fopen(argv[1], "r");
  if (!f) return 2;
  DecTables tb;
  for (int t = 0; t < 256; ++t) {
    Blk b{t};
    init_dec_tables(tb, b);
  }
  long n[3] = {0, 0, 0}, win[3] = {0, 0, 0}, bad = 0, tagbad = 0;
  char line[256];
  while (fgets(line, sizeof line, f)) {
    size_t len = strlen(line);
    while (len && (line[len - 1] == '\n' || line[len - 1] == '\r')) line[--len] = 0;
    if (len < 5) continue;
    const char kind = line[0];
    const bool tagw = line[2] == 'w';
    const std::string tok(line + 4);
    std::string s = tok;
    s += kind == 'f' ? ' ' : kind == 'i' ? ':' : ',';
    while (s.size() < 64) s += ' ';
    const uint8_t *p = reinterpret_cast<const uint8_t *>(s.data());
    uint32_t w[4];
    memcpy(w, p, 16);
    const uint64_t lim = 48;  // the chunk end: bytes at or past it read as NUL
    Src src;
    src.g = p;
    src.lim = lim;
    src.lds = p;
    src.wbase = 0;
    src.wend = s.size();
    GSrc at{p, lim};
    if (kind == 'f') {
      ++n[0];
      uint64_t e = 0;
      bool ne = false;
      const float r = parse_float(at, 0, &e, &ne);
      if (all_of(tok, "0123456789+-.eE")) {
        bool ok = false;
        const float v = wfloat32(w, tb, &ok);
        win[0] += ok;
        if (ok != tagw) {
          ++tagbad;
          if (bad++ < 20) printf("float tag '%s' tagged %c, wfloat32 ok %d\n", tok.c_str(), line[2], (int)ok);
        } else if (ok && memcmp(&v, &r, 4)) {
          if (bad++ < 20) printf("float value '%s' window %.9g byte %.9g\n", tok.c_str(), v, r);
        }
      } else if (tagw) {
        ++tagbad;
        if (bad++ < 20) printf("float tag '%s': outside the grammar, tagged window\n", tok.c_str());
      }
      bool ne1 = false;
      const float x = value_at(src, 0, &tb, &ne1);
      if (memcmp(&x, &r, 4) || ne1 != ne) {
        if (bad++ < 20) printf("value_at '%s' %.9g byte %.9g\n", tok.c_str(), x, r);
      }
      float cv;
      uint64_t ce = 0;
      if (csv_value_at(src, 0, &tb, &cv, &ce) && (memcmp(&cv, &r, 4) || ce != e)) {
        if (bad++ < 20) printf("csv_value_at '%s' %.9g end %llu byte %.9g end %llu\n", tok.c_str(), cv,
                               (unsigned long long)ce, r, (unsigned long long)e);
      }
    } else if (kind == 'i') {
      ++n[1];
      uint64_t v = 0, r32 = 0, r64 = 0;
      bool ok = false;
      const bool pos = wuint32(w, tb, &v, &ok);
      const bool p32 = parse_uint(at, 0, false, &r32), p64 = parse_uint(at, 0, true, &r64);
      const bool taken = ok && pos;  // svm_fast.h win_index, exact_dec.h index_at
      win[1] += taken;
      if (taken != tagw) {
        ++tagbad;
        if (bad++ < 20) printf("index tag '%s' tagged %c, wuint32 ok %d pos %d\n", tok.c_str(), line[2], (int)ok, (int)pos);
      } else if (taken && (!p32 || v != r32 || v != r64)) {
        if (bad++ < 20) printf("index value '%s' window %llu byte %llu / %llu\n", tok.c_str(), (unsigned long long)v,
                               (unsigned long long)r32, (unsigned long long)r64);
      }
      if (pos != p32 || pos != p64) {
        if (bad++ < 20) printf("index sign '%s'\n", tok.c_str());
      }
      for (int wide = 0; wide < 2; ++wide) {
        uint64_t a = 0;
        const bool pa = index_at(src, 0, wide, &tb, &a);
        if (pa != p32 || (pa && a != (wide ? r64 : r32))) {
          if (bad++ < 20) printf("index_at '%s' wide %d\n", tok.c_str(), wide);
        }
      }
    } else if (kind == 'n') {
      ++n[2];
      uint64_t e = 0;
      const int64_t r = c_strtoll(at, 0, 0, &e);
      if (all_of(tok, "0123456789+-")) {
        const uint32_t M = nd4(w[0]) | (nd4(w[1]) << 4) | (nd4(w[2]) << 8) | (nd4(w[3]) << 12);
        bool ok = false;
        const int64_t v = fcsv::wint64m(w, M, &ok);
        win[2] += ok;
        if (ok != tagw) {
          ++tagbad;
          if (bad++ < 20) printf("int tag '%s' tagged %c, wint64m ok %d\n", tok.c_str(), line[2], (int)ok);
        } else if (ok && (v != r || e != tok.size())) {
          if (bad++ < 20) printf("int value '%s' window %lld byte %lld\n", tok.c_str(), (long long)v, (long long)r);
        }
      } else if (tagw) {
        ++tagbad;
        if (bad++ < 20) printf("int tag '%s': outside the grammar, tagged window\n", tok.c_str());
      }
    }
  }
  fclose(f);
  printf("float %ld window %ld, index %ld window %ld, int %ld window %ld, tag mismatches %ld, mismatches %ld\n", n[0],
         win[0], n[1], win[1], n[2], win[2], tagbad, bad);
  return bad != 0;
}
