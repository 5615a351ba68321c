// capi.cpp -- the extern "C" boundary (include/dmlc_amd.h) over the HIP kernels.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "dmlc_amd.h"
#include "common.h"
#include "dmlc_amd_kernels.h"

namespace {

constexpr uint64_t kDefaultTile = 256ull << 10;  // bytes of text owned per workgroup (exact kernels)
constexpr uint64_t kFastTile = dmlc_amd::kFastTileBytes;  // fast_common.h kTile
constexpr int kSlots = 7;

uint64_t tile_of(const dmlc_amd_params *p) {
  return p && p->tile_bytes ? (uint64_t)p->tile_bytes : kDefaultTile;
}

struct Carve {
  char *p;
  size_t left;
  template <typename T>
  T *take(size_t n) {
    size_t bytes = (n * sizeof(T) + 255) & ~size_t(255);
    if (bytes > left) return nullptr;
    T *r = reinterpret_cast<T *>(p);
    p += bytes;
    left -= bytes;
    return r;
  }
};

// Delimiters that ParseFloat / strtoll can consume, which would make the field
// structure depend on decoding (csv_parser.h:99-127): handled by the exact
// per-line path instead of the field-parallel one.
bool csv_delim_fast(int d) {
  return dmlc_amd::csv_delim_plain((unsigned)d & 0xFFu);  // args.h
}

// What dmlc_amd_parse sets alike in the three exact argument blocks
// (LibsvmArgs, CsvArgs, LibfmArgs) ...
template <class A>
void fill_exact_common(A &a, const void *d_text, uint64_t nbytes, const uint64_t *ucs, uint64_t nunits,
                       const dmlc_amd::UnitLim &ul, uint64_t T, uint64_t ntiles, const dmlc_amd_params *prm,
                       const dmlc_amd_csr *out, uint64_t *tile_cnt, uint64_t *tile_base, uint64_t *chunk_tab,
                       uint64_t *res, uint32_t *gate, uint32_t *rec, uint32_t rec_win) {
  std::memset(&a, 0, sizeof(a));
  a.text = reinterpret_cast<const uint8_t *>(d_text);
  a.n = nbytes;
  a.cs = ucs;
  a.nchunk = (int)nunits;
  a.ul = ul;
  a.tile_bytes = T;
  a.ntiles = (uint32_t)ntiles;
  a.wide = prm->index_bits == 64;
  a.tile_cnt = tile_cnt;
  a.tile_base = tile_base;
  a.offset = out->offset;
  a.label = static_cast<decltype(a.label)>(out->label);  // DType: float but for CSV
  a.weight = out->weight;
  a.index = out->index;
  a.value = static_cast<decltype(a.value)>(out->value);
  for (int i = 0; i < 8; ++i) a.cap[i] = out->cap[i];
  a.chunk_tab = chunk_tab;
  a.err = reinterpret_cast<unsigned long long *>(res + 8);
  a.gate = gate;
  a.rec = rec;
  a.rec_win = rec ? rec_win : 0;
}
// ... and in the two single-pass ones (FastSvmArgs, FastCsvArgs)
template <class F>
void fill_fast_common(F &f, const void *d_text, uint64_t nbytes, const uint64_t *ucs, uint64_t nunits, uint64_t nft,
                      const dmlc_amd_params *prm, const dmlc_amd_csr *out, int phase, uint64_t *lb, uint32_t *gate,
                      unsigned long long *ferr, uint64_t *res) {
  std::memset(&f, 0, sizeof(f));
  f.text = reinterpret_cast<const uint8_t *>(d_text);
  f.n = nbytes;
  f.cs = ucs;
  f.nchunk = (int)nunits;
  f.ntiles = (uint32_t)nft;
  f.wide = prm->index_bits == 64;
  f.skip_if_gated = phase == dmlc_amd::kPhaseFill;
  f.offset = out->offset;
  f.label = reinterpret_cast<float *>(out->label);
  f.weight = out->weight;
  f.index = out->index;
  f.value = static_cast<decltype(f.value)>(out->value);
  for (int i = 0; i < 8; ++i) f.cap[i] = out->cap[i];
  f.lb = lb;
  f.gate = gate;
  f.err = ferr;
  f.res = res;
}

// ---- kernel timing (dmlc_amd_profile_begin / _end)
struct Profile {
  bool on = false;
  std::vector<hipEvent_t> ev;  // pairs: begin, end
  size_t used = 0;
  const char *kernel = "";
};
thread_local Profile g_prof;
thread_local hipError_t g_last_hip = hipSuccess;

}  // namespace

namespace dmlc_amd {
void prof_mark(int end, hipStream_t s, const char *kernel) {
  Profile &p = g_prof;
  if (!p.on) return;
  if (!end) {
    if (p.used + 2 > p.ev.size()) {
      for (int i = 0; i < 64; ++i) {
        hipEvent_t e;
        // no system-scope fence: a timing marker between kernels of one stream
        // (with it each marker cost the call about 5 us of GPU time)
        if (hipEventCreateWithFlags(&e, hipEventDisableSystemFence) != hipSuccess) return;
        p.ev.push_back(e);
      }
    }
    (void)hipEventRecord(p.ev[p.used], s);
    p.kernel = kernel;
  } else {
    (void)hipEventRecord(p.ev[p.used + 1], s);
    p.used += 2;
  }
}
}  // namespace dmlc_amd

extern "C" {

int dmlc_amd_profile_begin(void) {
  g_prof.on = true;
  g_prof.used = 0;
  return DMLC_AMD_OK;
}

int dmlc_amd_profile_end(double *total_ms, int *launches, const char **kernel) {
  Profile &p = g_prof;
  p.on = false;
  double t = 0;
  for (size_t i = 0; i + 1 < p.used; i += 2) {
    float ms = 0;
    if (hipEventSynchronize(p.ev[i + 1]) != hipSuccess ||
        hipEventElapsedTime(&ms, p.ev[i], p.ev[i + 1]) != hipSuccess)
      return DMLC_AMD_ERR_HIP;
    t += ms;
  }
  if (total_ms) *total_ms = t;
  if (launches) *launches = (int)(p.used / 2);
  if (kernel) *kernel = p.kernel;
  p.used = 0;
  return DMLC_AMD_OK;
}


int dmlc_amd_abi_version(void) { return DMLC_AMD_ABI_VERSION; }

#ifndef DMLC_AMD_BUILD_ID
#define DMLC_AMD_BUILD_ID "unknown"
#endif
const char *dmlc_amd_build_id(void) { return DMLC_AMD_BUILD_ID; }

int dmlc_amd_fast_geometry(uint32_t *tile_bytes, uint32_t *max_unit_starts) {
  if (tile_bytes) *tile_bytes = (uint32_t)dmlc_amd::kFastTileBytes;
  if (max_unit_starts) *max_unit_starts = (uint32_t)dmlc_amd::kFastMaxCs;
  return DMLC_AMD_OK;
}

int dmlc_amd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char *dmlc_amd_error_string(int code) {
  switch (code) {
    case DMLC_AMD_OK: return "ok";
    case DMLC_AMD_ERR_NEG_INDEX: return "Check failed: sign == true";
    case DMLC_AMD_ERR_NAN_LITERAL: return "Check failed: *p == ')': Invalid NAN literal";
    case DMLC_AMD_ERR_CSV_DELIM: return "Delimiter is not found in the line";
    case DMLC_AMD_ERR_CAPACITY: return "output capacity exceeded";
    case DMLC_AMD_ERR_ARG: return "invalid argument";
    case DMLC_AMD_ERR_HIP: return "HIP runtime error";
    default: return "unknown error";
  }
}

// FillData ranges per chunk (dmlc_amd_params.nthread; 0 = 1)
int units_per_chunk(const dmlc_amd_params *p) { return p && p->nthread > 1 ? p->nthread : 1; }
constexpr int kMaxNthread = 1 << 12;

// the exact kernels' count-pass records (args.h exact_rec_*): bytes, 0 when
// they would outgrow the text
uint64_t rec_bytes_of(uint64_t nbytes, uint64_t T, uint64_t ntiles, const dmlc_amd_params *prm) {
  if (!prm) return 0;
  const uint64_t b = dmlc_amd::exact_rec_bytes(ntiles, dmlc_amd::exact_rec_win(T, dmlc_amd::kWin), dmlc_amd::kThreads);
  return dmlc_amd::exact_rec_on(nbytes, b) ? b : 0;
}

// single-pass look-back words: the full kernel's [5 nft] + a reserved word; libsvm
// adds the lean kernel's [5 nft] + its poison word (libsvm.hip); CSV keeps
// one 8-word record per tile (csv_fast.h csv_look_back)
uint64_t lb_words_of(uint64_t nft, const dmlc_amd_params *prm) {
  if (prm && prm->format == DMLC_AMD_CSV) return nft * dmlc_amd::kCsvLbWords + 1;
  return prm && prm->format == DMLC_AMD_LIBSVM ? nft * 10 + 2 : nft * 5 + 1;
}

size_t dmlc_amd_workspace_bytes(uint64_t nbytes, int nchunks, const dmlc_amd_params *prm) {
  const uint64_t T = tile_of(prm);
  const uint64_t ntiles = (nbytes + T - 1) / T;
  const uint64_t nc = (nchunks > 0 ? (uint64_t)nchunks : 1) * (uint64_t)units_per_chunk(prm);
  const uint64_t nft = (nbytes + kFastTile - 1) / kFastTile;
  return (size_t)((2 * ntiles * kSlots + 2 * nc + nc * 8 + (nc + 1) + lb_words_of(nft, prm) + dmlc_amd::kLabShards * 8) *
                      sizeof(uint64_t) +
                  12 * 256 + rec_bytes_of(nbytes, T, ntiles, prm) + 2 * 256);
}

int dmlc_amd_parse(const void *d_text, uint64_t nbytes, const uint64_t *d_chunk_starts, int nchunks,
                   const dmlc_amd_params *prm, const dmlc_amd_csr *out, uint64_t *d_chunk_table,
                   void *d_workspace, size_t workspace_bytes, dmlc_amd_result *d_result,
                   void *stream) {
  if (!prm || !out || !d_result) return DMLC_AMD_ERR_ARG;
  if (prm->format < DMLC_AMD_LIBSVM || prm->format > DMLC_AMD_LIBFM) return DMLC_AMD_ERR_ARG;
  if (prm->index_bits != 32 && prm->index_bits != 64) return DMLC_AMD_ERR_ARG;
  if (prm->value_type < DMLC_AMD_F32 || prm->value_type > DMLC_AMD_I64) return DMLC_AMD_ERR_ARG;
  if (prm->format != DMLC_AMD_CSV && prm->value_type != DMLC_AMD_F32) return DMLC_AMD_ERR_ARG;
  if (nbytes && (!d_text || !d_chunk_starts || nchunks < 1)) return DMLC_AMD_ERR_ARG;
  if (prm->format == DMLC_AMD_CSV && prm->label_column >= 0 &&
      prm->label_column == prm->weight_column)
    return DMLC_AMD_ERR_ARG;  // csv_parser.h:59-60
  if (prm->nthread < 0 || prm->nthread > kMaxNthread) return DMLC_AMD_ERR_ARG;
  if (workspace_bytes < dmlc_amd_workspace_bytes(nbytes, nchunks, prm) || !d_workspace)
    return DMLC_AMD_ERR_ARG;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const uint64_t T = tile_of(prm);
  const uint64_t ntiles = (nbytes + T - 1) / T;
  const int upc = units_per_chunk(prm);
  const uint64_t nunits = (uint64_t)(nchunks > 0 ? nchunks : 0) * (uint64_t)upc;
  if (nunits > (uint64_t)INT32_MAX) return DMLC_AMD_ERR_ARG;
  const int nc = nunits > 0 ? (int)nunits : 1;
  Carve cv{reinterpret_cast<char *>(d_workspace), workspace_bytes};
  uint64_t *tile_cnt = cv.take<uint64_t>(ntiles * kSlots + 1);
  uint64_t *tile_base = cv.take<uint64_t>(ntiles * kSlots + 1);
  uint64_t *chunk_min = cv.take<uint64_t>(nc);
  uint64_t *fast_min = cv.take<uint64_t>(nc);  // single-pass write pass, indexing_mode < 0 (svm_fast.h umin_fix)
  uint64_t *chunk_sink = cv.take<uint64_t>((size_t)nc * 8);
  uint64_t *units = cv.take<uint64_t>((size_t)nc + 1);  // ParseBlock unit starts (nthread > 1)
  const uint64_t nft = (nbytes + kFastTile - 1) / kFastTile;
  uint32_t *ctl = cv.take<uint32_t>(4);               // gate, gate after the count phase, recount flag
  unsigned long long *ferr = cv.take<unsigned long long>(1);
  uint64_t *lb = cv.take<uint64_t>(lb_words_of(nft, prm));
  uint64_t *labsum = cv.take<uint64_t>(dmlc_amd::kLabShards * 8);
  const uint64_t recb = rec_bytes_of(nbytes, T, ntiles, prm);
  const uint32_t rec_win = dmlc_amd::exact_rec_win(T, dmlc_amd::kWin);
  uint64_t *rec_meta = recb ? cv.take<uint64_t>(ntiles * rec_win * 2) : nullptr;
  uint32_t *rec = recb ? cv.take<uint32_t>(ntiles * rec_win * 4 * dmlc_amd::kThreads) : nullptr;
  if (recb && (!rec || !rec_meta)) return DMLC_AMD_ERR_ARG;
  if (!tile_cnt || !tile_base || !chunk_min || !fast_min || !chunk_sink || !units || !ctl || !ferr || !lb || !labsum)
    return DMLC_AMD_ERR_ARG;
  // FillData's thread ranges become the units the kernels parse; the
  // decoders still read to the end of the InputSplit chunk (args.h UnitLim)
  const uint64_t *ucs = d_chunk_starts;
  if (upc > 1 && nbytes > 0) {
    const hipError_t re = dmlc_amd::launch_ranges(reinterpret_cast<const uint8_t *>(d_text), d_chunk_starts,
                                                  nchunks, upc, nbytes, units, s);
    if (re != hipSuccess) {
      g_last_hip = re;
      return DMLC_AMD_ERR_HIP;
    }
    ucs = units;
  }
  const dmlc_amd::UnitLim ul{d_chunk_starts, upc};
  uint64_t *res = reinterpret_cast<uint64_t *>(d_result);
  const bool count_only = (prm->flags & DMLC_AMD_FLAG_COUNT_ONLY) != 0;
  const bool fill_only = (prm->flags & DMLC_AMD_FLAG_FILL_ONLY) != 0;
  if (count_only && fill_only) return DMLC_AMD_ERR_ARG;
  const int phase = count_only ? dmlc_amd::kPhaseCount
                               : (fill_only ? dmlc_amd::kPhaseFill : dmlc_amd::kPhaseFull);
  hipError_t e = hipSuccess;
  uint64_t *tab = d_chunk_table ? d_chunk_table : chunk_sink;  // the exact kernels always write one
  const bool exact_flag = (prm->flags & DMLC_AMD_FLAG_EXACT) != 0;
  if (prm->format == DMLC_AMD_LIBSVM) {
    dmlc_amd::LibsvmArgs a;
    fill_exact_common(a, d_text, nbytes, ucs, nunits, ul, T, ntiles, prm, out, tile_cnt, tile_base, tab, res, ctl, rec,
                      rec_win);
    a.indexing_mode = prm->indexing_mode;
    a.qid = out->qid;
    a.chunk_min = chunk_min;
    a.rec_meta = rec_meta;
    dmlc_amd::FastSvmArgs f;
    fill_fast_common(f, d_text, nbytes, ucs, nunits, nft, prm, out, phase, lb, ctl, ferr, res);
    f.indexing_mode = prm->indexing_mode;
    f.qid = out->qid;
    // indexing_mode < 0 needs the units' index ranges after the write pass:
    // the chunk table, or the workspace's when the caller passes none
    f.chunk_tab = d_chunk_table ? d_chunk_table : (prm->indexing_mode < 0 ? chunk_sink : nullptr);
    f.lean_lb = lb + nft * dmlc_amd::kFastLbWords + 1;  // past the reserved word after lb's records (zeroed with lb)
    f.lean_poison = f.lean_lb + nft * dmlc_amd::kFastLbWords;
    f.qsum = labsum;
    f.umin = fast_min;
    e = dmlc_amd::launch_libsvm(a, f, nbytes > 0 && !exact_flag, res, phase, s);
  } else if (prm->format == DMLC_AMD_CSV) {
    dmlc_amd::CsvArgs a;
    fill_exact_common(a, d_text, nbytes, ucs, nunits, ul, T, ntiles, prm, out, tile_cnt, tile_base, tab, res, ctl, rec,
                      rec_win);
    a.vtype = prm->value_type;
    a.label_column = prm->label_column;
    a.weight_column = prm->weight_column;
    a.delim = (uint32_t)prm->delimiter & 0xFFu;
    a.fast_delim = csv_delim_fast(prm->delimiter);
    dmlc_amd::FastCsvArgs f;
    fill_fast_common(f, d_text, nbytes, ucs, nunits, nft, prm, out, phase, lb, ctl, ferr, res);
    f.delim = a.delim;
    f.label_col = prm->label_column;
    // the weight column is ordinary for integer DTypes (csv_parser.h:113-114)
    f.weight_col = prm->value_type == DMLC_AMD_F32 ? prm->weight_column : -1;
    f.vtype = prm->value_type;
    f.labsum = labsum;
    f.chunk_tab = d_chunk_table;
    // the uniform-grammar CSV kernels: the label / weight columns they take
    // by DType, and a delimiter the number decoders cannot consume or ' ' /
    // '\t' (the whitespace mode); a.fast_delim stays the exact kernels' own
    // question (args.h csv_single_pass_*, csv_fast.h)
    const int sp_delim = dmlc_amd::csv_single_pass_delim(a.delim);
    f.ws = sp_delim == 2;
    const bool cols_ok = dmlc_amd::csv_single_pass_columns(prm->value_type, prm->label_column, prm->weight_column);
    e = dmlc_amd::launch_csv(a, f, nbytes > 0 && cols_ok && sp_delim != 0 && !exact_flag, res, phase, s);
  } else {  // DMLC_AMD_LIBFM
    dmlc_amd::LibfmArgs a;
    fill_exact_common(a, d_text, nbytes, ucs, nunits, ul, T, ntiles, prm, out, tile_cnt, tile_base, tab, res, ctl, rec,
                      rec_win);
    a.indexing_mode = prm->indexing_mode;
    a.field = out->field;
    a.chunk_min = chunk_min;
    a.rec_meta = rec_meta;
    dmlc_amd::FastSvmArgs f;  // the single-pass kernel with the libfm roles (svm_fast.h)
    fill_fast_common(f, d_text, nbytes, ucs, nunits, nft, prm, out, phase, lb, ctl, ferr, res);
    f.indexing_mode = prm->indexing_mode;
    f.field = out->field;
    f.chunk_tab = prm->indexing_mode < 0 ? tab : d_chunk_table;  // as libsvm's
    f.umin = fast_min;
    e = dmlc_amd::launch_libfm(a, f, nbytes > 0 && !exact_flag, res, phase, s);
  }
  if (e == hipSuccess && (prm->flags & DMLC_AMD_FLAG_MAX_INDEX) && phase != dmlc_amd::kPhaseCount) {
    // NumCol of the reference's BasicRowIter: maxima of what was written
    const int wide = prm->index_bits == 64;
    e = dmlc_amd::launch_max(out->index, wide, res + DMLC_AMD_INDEX, out->cap[DMLC_AMD_INDEX], res + 10, s);
    if (e == hipSuccess)
      e = dmlc_amd::launch_max(out->field, wide, res + DMLC_AMD_FIELD, out->cap[DMLC_AMD_FIELD], res + 11, s);
  }
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

int dmlc_amd_dense_geometry(uint32_t *cells_per_tile, uint32_t *rows_per_tile) {
  if (cells_per_tile) *cells_per_tile = dmlc_amd::kDenseCells;
  if (rows_per_tile) *rows_per_tile = dmlc_amd::kDenseRows;
  return DMLC_AMD_OK;
}

int dmlc_amd_to_dense(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result,
                      const dmlc_amd_dense_params *prm, void *d_out, uint64_t *d_status, void *stream) {
  if (!csr || !d_result || !prm || !d_out || !d_status) return DMLC_AMD_ERR_ARG;
  if (prm->index_bits != 32 && prm->index_bits != 64) return DMLC_AMD_ERR_ARG;
  if (prm->value_type < DMLC_AMD_F32 || prm->value_type > DMLC_AMD_I64) return DMLC_AMD_ERR_ARG;
  if (prm->ncol == 0 || prm->ld < prm->ncol) return DMLC_AMD_ERR_ARG;
  const int vbytes = prm->value_type == DMLC_AMD_I64 ? 8 : 4;
  if (reinterpret_cast<uintptr_t>(d_out) % (uintptr_t)vbytes) return DMLC_AMD_ERR_ARG;
  // the rows the window can hold: the parsed count is known on the device
  // only, so tiles are launched for all of them and leave early past it
  const uint64_t cap_rows = csr->cap[DMLC_AMD_ROWS];
  const uint64_t nrows = prm->row_begin < cap_rows ? dmlc_amd::mn<uint64_t>(prm->max_rows, cap_rows - prm->row_begin) : 0;
  if (nrows && (!csr->offset || (csr->cap[DMLC_AMD_INDEX] && !csr->index))) return DMLC_AMD_ERR_ARG;
  dmlc_amd::DenseArgs a;
  std::memset(&a, 0, sizeof(a));
  dmlc_amd::dense_shape(prm->ncol, &a.S, &a.R);
  const uint64_t col_tiles = (prm->ncol - 1) / a.S + 1;
  const uint64_t row_tiles = nrows ? (nrows - 1) / a.R + 1 : 0;
  // never truncated: a window of more tiles than the grid holds is refused
  if (col_tiles > dmlc_amd::kDenseMaxTiles || row_tiles > dmlc_amd::kDenseMaxTiles ||
      col_tiles * row_tiles > dmlc_amd::kDenseMaxTiles)
    return DMLC_AMD_ERR_ARG;
  a.offset = csr->offset;
  a.index = csr->index;
  a.value = csr->value;
  a.res = reinterpret_cast<const uint64_t *>(d_result);
  a.cap_rows = cap_rows;
  a.cap_index = csr->cap[DMLC_AMD_INDEX];
  // (without a value array the kernel reads none: count[VALUE] == 0 gives ones)
  a.cap_value = csr->value ? csr->cap[DMLC_AMD_VALUE] : 0;
  a.row_begin = prm->row_begin;
  a.row_end = prm->row_begin + prm->max_rows < prm->row_begin ? ~0ull : prm->row_begin + prm->max_rows;
  a.ncol = prm->ncol;
  a.ld = prm->ld;
  a.fill = vbytes == 8 ? prm->fill_bits : (prm->fill_bits & 0xFFFFFFFFull);
  a.one = prm->value_type == DMLC_AMD_F32 ? 0x3F800000ull : 1ull;
  a.col_tiles = (uint32_t)col_tiles;
  a.out = d_out;
  a.status = d_status;
  const hipError_t e = dmlc_amd::launch_dense(a, prm->index_bits == 64, vbytes, (uint32_t)(col_tiles * row_tiles),
                                              reinterpret_cast<hipStream_t>(stream));
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

int dmlc_amd_gather_geometry(uint32_t *rows_per_tile) {
  if (rows_per_tile) *rows_per_tile = dmlc_amd::kGatherRows;
  return DMLC_AMD_OK;
}

// one record per tile of ids (gather_core.h), in whole 256-byte lines
size_t dmlc_amd_gather_workspace_bytes(uint64_t n_ids) {
  const uint64_t ntiles = n_ids / dmlc_amd::kGatherRows + (n_ids % dmlc_amd::kGatherRows != 0);
  return (size_t)(((ntiles * dmlc_amd::kGatherRecWords * sizeof(uint64_t) + 255) & ~255ull) + 256);
}

namespace {
// the arrays of one side as the kernels take them: a null array holds nothing
dmlc_amd::GatherCsr gather_side(const dmlc_amd_csr *c) {
  dmlc_amd::GatherCsr g;
  std::memset(&g, 0, sizeof(g));
  g.offset = c->offset;
  g.label = c->label;
  g.weight = reinterpret_cast<uint32_t *>(c->weight);
  g.qid = c->qid;
  g.field = c->field;
  g.index = c->index;
  g.value = c->value;
  g.cap[DMLC_AMD_ROWS] = c->offset ? c->cap[DMLC_AMD_ROWS] : 0;
  g.cap[DMLC_AMD_LABEL] = c->label ? g.cap[DMLC_AMD_ROWS] : 0;  // cap[ROWS] counts labels
  g.cap[DMLC_AMD_WEIGHT] = c->weight ? c->cap[DMLC_AMD_WEIGHT] : 0;
  g.cap[DMLC_AMD_QID] = c->qid ? c->cap[DMLC_AMD_QID] : 0;
  g.cap[DMLC_AMD_INDEX] = c->index ? c->cap[DMLC_AMD_INDEX] : 0;
  g.cap[DMLC_AMD_VALUE] = c->value ? c->cap[DMLC_AMD_VALUE] : 0;
  g.cap[DMLC_AMD_FIELD] = c->field ? c->cap[DMLC_AMD_FIELD] : 0;
  return g;
}
bool same_array(const void *a, const void *b) { return a != nullptr && a == b; }
}  // namespace

int dmlc_amd_gather_rows(const dmlc_amd_csr *src, const dmlc_amd_result *d_src_result, const void *d_ids,
                         uint64_t n_ids, const dmlc_amd_gather_params *prm, const dmlc_amd_csr *dst,
                         dmlc_amd_result *d_dst_result, uint64_t *d_status, void *d_workspace,
                         size_t workspace_bytes, void *stream) {
  if (!src || !d_src_result || !prm || !dst || !d_dst_result || !d_status || !d_workspace) return DMLC_AMD_ERR_ARG;
  if (n_ids && !d_ids) return DMLC_AMD_ERR_ARG;
  if (!dst->offset) return DMLC_AMD_ERR_ARG;  // dst.offset[0] is always written
  if (prm->index_bits != 32 && prm->index_bits != 64) return DMLC_AMD_ERR_ARG;
  if (prm->id_bits != 32 && prm->id_bits != 64) return DMLC_AMD_ERR_ARG;
  if (prm->value_type < DMLC_AMD_F32 || prm->value_type > DMLC_AMD_I64) return DMLC_AMD_ERR_ARG;
  if (prm->label_type < DMLC_AMD_F32 || prm->label_type > DMLC_AMD_I64) return DMLC_AMD_ERR_ARG;
  if (prm->flags & ~DMLC_AMD_FLAG_MAX_INDEX) return DMLC_AMD_ERR_ARG;
  if (prm->reserved[0] || prm->reserved[1] || prm->reserved[2]) return DMLC_AMD_ERR_ARG;
  const uint64_t ntiles = n_ids / dmlc_amd::kGatherRows + (n_ids % dmlc_amd::kGatherRows != 0);
  // never truncated: more ids than the grid holds tiles for are refused
  if (ntiles > dmlc_amd::kGatherMaxTiles) return DMLC_AMD_ERR_ARG;
  if (workspace_bytes < dmlc_amd_gather_workspace_bytes(n_ids)) return DMLC_AMD_ERR_ARG;
  if (same_array(src->offset, dst->offset) || same_array(src->label, dst->label) ||
      same_array(src->weight, dst->weight) || same_array(src->qid, dst->qid) || same_array(src->field, dst->field) ||
      same_array(src->index, dst->index) || same_array(src->value, dst->value) ||
      same_array(d_src_result, d_dst_result))
    return DMLC_AMD_ERR_ARG;
  dmlc_amd::GatherArgs a;
  std::memset(&a, 0, sizeof(a));
  a.src = gather_side(src);
  a.dst = gather_side(dst);
  a.res = reinterpret_cast<const uint64_t *>(d_src_result);
  a.dres = reinterpret_cast<uint64_t *>(d_dst_result);
  a.ids = d_ids;
  a.n_ids = n_ids;
  a.ntiles = ntiles;
  a.id_wide = prm->id_bits == 64;
  a.label_bytes = prm->label_type == DMLC_AMD_I64 ? 8 : 4;
  a.rec = reinterpret_cast<uint64_t *>(d_workspace);
  a.status = d_status;
  hipStream_t s = reinterpret_cast<hipStream_t>(stream);
  const int wide = prm->index_bits == 64;
  hipError_t e = dmlc_amd::launch_gather(a, wide, prm->value_type == DMLC_AMD_I64 ? 8 : 4, s);
  if (e == hipSuccess && (prm->flags & DMLC_AMD_FLAG_MAX_INDEX)) {
    // maxima of what was written, as after a parse
    e = dmlc_amd::launch_max(a.dst.index, wide, a.dres + DMLC_AMD_INDEX, a.dst.cap[DMLC_AMD_INDEX], a.dres + 10, s);
    if (e == hipSuccess)
      e = dmlc_amd::launch_max(a.dst.field, wide, a.dres + DMLC_AMD_FIELD, a.dst.cap[DMLC_AMD_FIELD], a.dres + 11, s);
  }
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

int dmlc_amd_csc_geometry(uint32_t *entries_per_tile, uint32_t *radix_bits) {
  if (entries_per_tile) *entries_per_tile = dmlc_amd::kCscTile;
  if (radix_bits) *radix_bits = dmlc_amd::kCscRadixBits;
  return DMLC_AMD_OK;
}

namespace {
// the workspace of a CSC call (csc_core.h), every part in whole 256-byte lines:
// meta, the digit totals, the tile records, the histogram, and with more than
// one pass the two payload buffers (the second holds only columns for two passes)
struct CscLayout {
  uint64_t ntiles, passes;
  uint64_t total, rec, hist, buf[2][4];  // byte offsets; buf[b] = col, row, rpos, val
  uint64_t bytes;
};
bool csc_prm_ok(const dmlc_amd_csc_params *prm) {
  if (!prm) return false;
  if (prm->index_bits != 32 && prm->index_bits != 64) return false;
  if (prm->value_type < DMLC_AMD_F32 || prm->value_type > DMLC_AMD_I64) return false;
  if (prm->ncol == 0 || prm->ncol > (1ull << 32)) return false;
  if (prm->flags || prm->reserved[0] || prm->reserved[1] || prm->reserved[2]) return false;
  return true;
}
CscLayout csc_layout(uint64_t m, uint64_t ncol, int vbytes) {
  CscLayout L;
  std::memset(&L, 0, sizeof(L));
  auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
  L.ntiles = m / dmlc_amd::kCscTile + (m % dmlc_amd::kCscTile != 0);
  if (L.ntiles == 0) L.ntiles = 1;  // the first tile also stores col_offset
  L.passes = dmlc_amd::csc_passes(ncol);
  uint64_t at = 256;  // meta
  L.total = at;
  at += up(dmlc_amd::kCscDigits * 4);
  L.rec = at;
  at += up(L.ntiles * dmlc_amd::kCscRecWords * 8);
  L.hist = at;
  at += up(L.ntiles * dmlc_amd::kCscDigits * 4);
  if (L.passes > 1)
    for (int b = 0; b < 2; ++b) {
      const bool full = b == 0 || L.passes > 2;
      L.buf[b][0] = at;
      at += up(m * 4);
      if (!full) continue;
      L.buf[b][1] = at;
      at += up(m * 4);
      L.buf[b][2] = at;
      at += up(m * 4);
      L.buf[b][3] = at;
      at += up(m * (uint64_t)vbytes);
    }
  L.bytes = at;
  return L;
}
}  // namespace

size_t dmlc_amd_csc_workspace_bytes(uint64_t max_entries, uint64_t ncol, const dmlc_amd_csc_params *prm) {
  if (!csc_prm_ok(prm) || ncol == 0 || ncol > (1ull << 32) || max_entries >= dmlc_amd::kCscMaxWindow) return 0;
  return (size_t)csc_layout(max_entries, ncol, prm->value_type == DMLC_AMD_I64 ? 8 : 4).bytes;
}

int dmlc_amd_to_csc(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_csc_params *prm,
                    const dmlc_amd_csc *csc, uint64_t *d_status, void *d_workspace, size_t workspace_bytes,
                    void *stream) {
  if (!csr || !d_result || !prm || !csc || !d_status || !d_workspace) return DMLC_AMD_ERR_ARG;
  if (!csc->col_offset || !csc->row) return DMLC_AMD_ERR_ARG;
  if (!csc_prm_ok(prm)) return DMLC_AMD_ERR_ARG;
  // the rows and entries the window can hold: the parsed counts are known on
  // the device only, so tiles are launched for the bound and leave early past them
  const uint64_t cap_rows = csr->offset ? csr->cap[DMLC_AMD_ROWS] : 0;
  const uint64_t cap_index = csr->index ? csr->cap[DMLC_AMD_INDEX] : 0;
  const uint64_t nrows = prm->row_begin < cap_rows ? dmlc_amd::mn<uint64_t>(prm->max_rows, cap_rows - prm->row_begin) : 0;
  const uint64_t m = prm->max_entries ? dmlc_amd::mn<uint64_t>(prm->max_entries, cap_index) : cap_index;
  if (nrows >= dmlc_amd::kCscMaxWindow || m >= dmlc_amd::kCscMaxWindow) return DMLC_AMD_ERR_ARG;
  const int vbytes = prm->value_type == DMLC_AMD_I64 ? 8 : 4;
  const CscLayout L = csc_layout(m, prm->ncol, vbytes);
  if (workspace_bytes < L.bytes) return DMLC_AMD_ERR_ARG;
  const void *srcs[] = {csr->offset, csr->label, csr->weight, csr->qid, csr->field, csr->index, csr->value, d_result};
  const void *outs[] = {csc->col_offset, csc->row, csc->value, csc->pos, d_status, d_workspace};
  for (const void *o : outs)
    for (const void *s : srcs)
      if (same_array(o, s)) return DMLC_AMD_ERR_ARG;
  dmlc_amd::CscArgs a;
  std::memset(&a, 0, sizeof(a));
  a.offset = csr->offset;
  a.index = csr->index;
  a.value = csr->value;
  a.res = reinterpret_cast<const uint64_t *>(d_result);
  a.cap_rows = cap_rows;
  a.cap_index = cap_index;
  a.cap_value = csr->value ? csr->cap[DMLC_AMD_VALUE] : 0;
  a.row_begin = prm->row_begin;
  a.row_end = prm->row_begin + prm->max_rows < prm->row_begin ? ~0ull : prm->row_begin + prm->max_rows;
  a.ncol = prm->ncol;
  a.max_entries = m;
  a.ntiles = L.ntiles;
  a.passes = (uint32_t)L.passes;
  a.col_offset = csc->col_offset;
  a.row = csc->row;
  a.val = csc->value;
  a.pos = csc->pos;
  a.cap = csc->cap;
  a.status = d_status;
  char *ws = static_cast<char *>(d_workspace);
  a.meta = reinterpret_cast<uint64_t *>(ws);
  a.total = reinterpret_cast<uint32_t *>(ws + L.total);
  a.rec = reinterpret_cast<uint64_t *>(ws + L.rec);
  a.hist = reinterpret_cast<uint32_t *>(ws + L.hist);
  if (L.passes > 1)
    for (int b = 0; b < 2; ++b) {
      a.buf[b].col = reinterpret_cast<uint32_t *>(ws + L.buf[b][0]);
      if (b == 1 && L.passes == 2) continue;
      a.buf[b].row = reinterpret_cast<uint32_t *>(ws + L.buf[b][1]);
      a.buf[b].rpos = reinterpret_cast<uint32_t *>(ws + L.buf[b][2]);
      a.buf[b].val = ws + L.buf[b][3];
    }
  const hipError_t e = dmlc_amd::launch_csc(a, prm->index_bits == 64, vbytes, reinterpret_cast<hipStream_t>(stream));
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

int dmlc_amd_bins_geometry(uint32_t *cells_per_tile, uint32_t *rows_per_tile) {
  return dmlc_amd_dense_geometry(cells_per_tile, rows_per_tile);  // the dense tile (bins_core.h)
}

int dmlc_amd_to_bins(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_cuts *cuts,
                     const dmlc_amd_bins_params *prm, void *d_out, uint64_t *d_status, void *stream) {
  if (!csr || !d_result || !cuts || !prm || !d_out || !d_status) return DMLC_AMD_ERR_ARG;
  if (!cuts->cut_ptr || (cuts->n_cuts && !cuts->cut_value)) return DMLC_AMD_ERR_ARG;
  if (prm->index_bits != 32 && prm->index_bits != 64) return DMLC_AMD_ERR_ARG;
  if (prm->value_type != DMLC_AMD_F32) return DMLC_AMD_ERR_ARG;
  const int cbytes = prm->code_bytes;
  if (cbytes != 1 && cbytes != 2 && cbytes != 4) return DMLC_AMD_ERR_ARG;
  if (cbytes < 4 && (prm->missing_code >> (8 * cbytes)) != 0) return DMLC_AMD_ERR_ARG;
  if (prm->ncol == 0 || prm->ncol >= (1ull << 32) || prm->ld < prm->ncol) return DMLC_AMD_ERR_ARG;
  if (prm->flags & ~DMLC_AMD_BINS_GLOBAL) return DMLC_AMD_ERR_ARG;
  if (prm->reserved[0] || prm->reserved[1] || prm->reserved[2]) return DMLC_AMD_ERR_ARG;
  if (reinterpret_cast<uintptr_t>(d_out) % (uintptr_t)cbytes) return DMLC_AMD_ERR_ARG;
  const void *srcs[] = {csr->offset, csr->label,       csr->weight,     csr->qid, csr->field, csr->index,
                        csr->value,  d_result,         cuts->cut_ptr,   cuts->cut_value};
  for (const void *s : srcs)
    if (same_array(d_out, s) || same_array(d_status, s)) return DMLC_AMD_ERR_ARG;
  // the rows the window can hold, as in dmlc_amd_to_dense
  const uint64_t cap_rows = csr->cap[DMLC_AMD_ROWS];
  const uint64_t nrows = prm->row_begin < cap_rows ? dmlc_amd::mn<uint64_t>(prm->max_rows, cap_rows - prm->row_begin) : 0;
  if (nrows && (!csr->offset || (csr->cap[DMLC_AMD_INDEX] && !csr->index))) return DMLC_AMD_ERR_ARG;
  dmlc_amd::BinsArgs b;
  std::memset(&b, 0, sizeof(b));
  dmlc_amd::DenseArgs &a = b.d;
  dmlc_amd::dense_shape(prm->ncol, &a.S, &a.R);
  const uint64_t col_tiles = (prm->ncol - 1) / a.S + 1;
  const uint64_t row_tiles = nrows ? (nrows - 1) / a.R + 1 : 0;
  // never truncated: a window of more tiles than the grid holds is refused
  if (col_tiles > dmlc_amd::kDenseMaxTiles || row_tiles > dmlc_amd::kDenseMaxTiles ||
      col_tiles * row_tiles > dmlc_amd::kDenseMaxTiles)
    return DMLC_AMD_ERR_ARG;
  a.offset = csr->offset;
  a.index = csr->index;
  a.value = csr->value;
  a.res = reinterpret_cast<const uint64_t *>(d_result);
  a.cap_rows = cap_rows;
  a.cap_index = csr->cap[DMLC_AMD_INDEX];
  a.cap_value = csr->value ? csr->cap[DMLC_AMD_VALUE] : 0;
  a.row_begin = prm->row_begin;
  a.row_end = prm->row_begin + prm->max_rows < prm->row_begin ? ~0ull : prm->row_begin + prm->max_rows;
  a.ncol = prm->ncol;
  a.ld = prm->ld;
  a.one = 0x3F800000ull;
  a.col_tiles = (uint32_t)col_tiles;
  a.out = d_out;
  a.status = d_status;
  b.cut_ptr = cuts->cut_ptr;
  b.cut_value = cuts->cut_value;
  b.n_cuts = cuts->n_cuts;
  b.missing = prm->missing_code;
  b.global_ids = (prm->flags & DMLC_AMD_BINS_GLOBAL) != 0;
  const hipError_t e = dmlc_amd::launch_bins(b, prm->index_bits == 64, cbytes, (uint32_t)(col_tiles * row_tiles),
                                             reinterpret_cast<hipStream_t>(stream));
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

int dmlc_amd_make_cuts_geometry(uint32_t *entries_per_tile, uint32_t *radix_bits) {
  if (entries_per_tile) *entries_per_tile = dmlc_amd::kCutsTile;
  if (radix_bits) *radix_bits = dmlc_amd::kCutsRadixBits;
  return DMLC_AMD_OK;
}

namespace {
// the workspace of a make_cuts call (cuts_core.h), every part in whole 256-byte
// lines: meta, the digit totals, the tile records, the histogram, the two
// (column, key) buffers, and each column's first sorted entry and sample count
struct CutsLayout {
  uint64_t ntiles, passes;
  uint64_t total, rec, hist, col[2], key[2], cstart, cn;  // byte offsets
  uint64_t bytes;
};
bool cuts_prm_ok(const dmlc_amd_make_cuts_params *prm) {
  if (!prm) return false;
  if (prm->index_bits != 32 && prm->index_bits != 64) return false;
  if (prm->value_type != DMLC_AMD_F32) return false;
  if (prm->ncol == 0 || prm->max_bin == 0) return false;
  if (prm->ncol >= (1ull << 32) || prm->ncol * (uint64_t)prm->max_bin >= (1ull << 32)) return false;
  if (prm->flags || prm->reserved[0] || prm->reserved[1]) return false;
  return true;
}
CutsLayout cuts_layout(uint64_t m, uint64_t ncol) {
  CutsLayout L;
  std::memset(&L, 0, sizeof(L));
  auto up = [](uint64_t b) { return (b + 255) & ~255ull; };
  L.ntiles = m / dmlc_amd::kCutsTile + (m % dmlc_amd::kCutsTile != 0);
  if (L.ntiles == 0) L.ntiles = 1;
  L.passes = dmlc_amd::kCutsKeyPasses + dmlc_amd::cuts_col_passes(ncol);
  uint64_t at = 256;  // meta
  L.total = at;
  at += up(dmlc_amd::kCutsDigits * 4);
  L.rec = at;
  at += up(L.ntiles * dmlc_amd::kCutsRecWords * 8);
  L.hist = at;
  at += up(L.ntiles * dmlc_amd::kCutsDigits * 4);
  for (int b = 0; b < 2; ++b) {
    L.col[b] = at;
    at += up(m * 4);
    L.key[b] = at;
    at += up(m * 4);
  }
  L.cstart = at;
  at += up((ncol + 1) * 4);
  L.cn = at;
  at += up(ncol * 4);
  L.bytes = at;
  return L;
}
}  // namespace

size_t dmlc_amd_make_cuts_workspace_bytes(uint64_t max_entries, uint64_t ncol, const dmlc_amd_make_cuts_params *prm) {
  if (!cuts_prm_ok(prm) || ncol == 0 || ncol * (uint64_t)prm->max_bin >= (1ull << 32) || ncol >= (1ull << 32) ||
      max_entries >= dmlc_amd::kCutsMaxWindow)
    return 0;
  return (size_t)cuts_layout(max_entries, ncol).bytes;
}

int dmlc_amd_make_cuts(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_make_cuts_params *prm,
                       const dmlc_amd_cuts_out *out, uint64_t *d_status, void *d_workspace, size_t workspace_bytes,
                       void *stream) {
  if (!csr || !d_result || !prm || !out || !d_status || !d_workspace) return DMLC_AMD_ERR_ARG;
  if (!out->cut_ptr || (out->cap && !out->cut_value)) return DMLC_AMD_ERR_ARG;
  if (!cuts_prm_ok(prm)) return DMLC_AMD_ERR_ARG;
  // the rows and entries the window can hold: the parsed counts are known on
  // the device only, so tiles are launched for the bound and leave early past them
  const uint64_t cap_rows = csr->offset ? csr->cap[DMLC_AMD_ROWS] : 0;
  const uint64_t cap_index = csr->index ? csr->cap[DMLC_AMD_INDEX] : 0;
  const uint64_t nrows = prm->row_begin < cap_rows ? dmlc_amd::mn<uint64_t>(prm->max_rows, cap_rows - prm->row_begin) : 0;
  const uint64_t m = prm->max_entries ? dmlc_amd::mn<uint64_t>(prm->max_entries, cap_index) : cap_index;
  if (nrows >= dmlc_amd::kCutsMaxWindow || m >= dmlc_amd::kCutsMaxWindow) return DMLC_AMD_ERR_ARG;
  const CutsLayout L = cuts_layout(m, prm->ncol);
  if (workspace_bytes < L.bytes) return DMLC_AMD_ERR_ARG;
  const void *srcs[] = {csr->offset, csr->label, csr->weight, csr->qid, csr->field, csr->index, csr->value, d_result};
  const void *outs[] = {out->cut_ptr, out->cut_value, d_status, d_workspace};
  for (const void *o : outs)
    for (const void *s : srcs)
      if (same_array(o, s)) return DMLC_AMD_ERR_ARG;
  dmlc_amd::MakeCutsArgs a;
  std::memset(&a, 0, sizeof(a));
  a.offset = csr->offset;
  a.index = csr->index;
  a.value = reinterpret_cast<const uint32_t *>(csr->value);
  a.res = reinterpret_cast<const uint64_t *>(d_result);
  a.cap_rows = cap_rows;
  a.cap_index = cap_index;
  a.cap_value = csr->value ? csr->cap[DMLC_AMD_VALUE] : 0;
  a.row_begin = prm->row_begin;
  a.row_end = prm->row_begin + prm->max_rows < prm->row_begin ? ~0ull : prm->row_begin + prm->max_rows;
  a.ncol = prm->ncol;
  a.max_entries = m;
  a.ntiles = L.ntiles;
  a.max_bin = prm->max_bin;
  a.passes = (uint32_t)L.passes;
  a.cut_ptr = out->cut_ptr;
  a.cut_value = reinterpret_cast<uint32_t *>(out->cut_value);
  a.cap = out->cap;
  a.status = d_status;
  char *ws = static_cast<char *>(d_workspace);
  a.meta = reinterpret_cast<uint64_t *>(ws);
  a.total = reinterpret_cast<uint32_t *>(ws + L.total);
  a.rec = reinterpret_cast<uint64_t *>(ws + L.rec);
  a.hist = reinterpret_cast<uint32_t *>(ws + L.hist);
  for (int b = 0; b < 2; ++b) {
    a.col[b] = reinterpret_cast<uint32_t *>(ws + L.col[b]);
    a.key[b] = reinterpret_cast<uint32_t *>(ws + L.key[b]);
  }
  a.cstart = reinterpret_cast<uint32_t *>(ws + L.cstart);
  a.cn = reinterpret_cast<uint32_t *>(ws + L.cn);
  const hipError_t e = dmlc_amd::launch_make_cuts(a, prm->index_bits == 64, reinterpret_cast<hipStream_t>(stream));
  g_last_hip = e;
  return e == hipSuccess ? DMLC_AMD_OK : DMLC_AMD_ERR_HIP;
}

const char *dmlc_amd_last_hip_error(void) { return hipGetErrorString(g_last_hip); }

}  // extern "C"
