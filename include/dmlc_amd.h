/*
 * dmlc_amd.h -- C ABI of the MI355X text -> CSR parse path.
 *
 * This is the drop-in boundary below dmlc-core's parser plugin API.  The host
 * side (dmlc::Parser<I,D>::Create, src/data.cc:152-186, and the text parsers
 * registered at src/data.cc:202-221) hands InputSplit chunks to these entry
 * points; each replaces the CPU ParseBlock of one parser:
 *
 *   format DMLC_AMD_LIBSVM -> LibSVMParser<I>::ParseBlock  (src/data/libsvm_parser.h:85-172)
 *   format DMLC_AMD_CSV    -> CSVParser<I,D>::ParseBlock   (src/data/csv_parser.h:71-149)
 *   format DMLC_AMD_LIBFM  -> LibFMParser<I>::ParseBlock   (src/data/libfm_parser.h:67-144)
 *
 * Semantics: the text buffer holds `nchunks` consecutive InputSplit chunks
 * (chunk c = [chunk_starts[c], chunk_starts[c+1]), chunk_starts[nchunks] ==
 * nbytes).  Each chunk goes through TextParserBase::FillData
 * (text_parser.h:116-155): it is cut into T = max(params.nthread, 1) ranges
 * (BackFindEndLine, text_parser.h:70-77) and each range is parsed as ONE
 * ParseBlock -- a "unit"; unit u = c * T + t.  The per-unit
 * RowBlockContainers are returned concatenated, exactly as
 * RowBlockContainer::Push(RowBlock) (src/data/row_block.h:126-168) would
 * concatenate them: offsets are global.  Per-unit boundaries are reported in
 * chunk_table so the caller can rebuild the per-unit RowBlock views (the
 * reference's blocks, parser.h:32-48) and run GetBlock's consistency CHECKs
 * (row_block.h:171-189) per unit.  T changes the result only through
 * indexing_mode < 0, whose 1-based detection is per unit
 * (libsvm_parser.h:165-171, libfm_parser.h likewise).
 *
 * All pointers named d_* and every pointer inside dmlc_amd_csr are DEVICE
 * pointers.  Calls are asynchronous on `stream` (a hipStream_t, NULL = default
 * stream); results land in *d_result.  No host synchronisation, allocation or
 * device-wide barrier happens inside a call, so calls can be captured into a
 * hipGraph.  Only plain pointers and sizes cross this boundary.
 */
#ifndef DMLC_AMD_H_
#define DMLC_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DMLC_AMD_ABI_VERSION 2

enum { DMLC_AMD_LIBSVM = 0, DMLC_AMD_CSV = 1, DMLC_AMD_LIBFM = 2 };
enum { DMLC_AMD_F32 = 0, DMLC_AMD_I32 = 1, DMLC_AMD_I64 = 2 };

/* counter slots of dmlc_amd_result.count / chunk_table rows / csr.cap */
enum {
  DMLC_AMD_ROWS = 0,   /* rows (RowBlock::size); offset has rows + 1 entries */
  DMLC_AMD_INDEX = 1,  /* feature indices (RowBlock::index) */
  DMLC_AMD_VALUE = 2,  /* values (RowBlock::value); 0 when the input has none */
  DMLC_AMD_WEIGHT = 3, /* instance weights (RowBlock::weight) */
  DMLC_AMD_QID = 4,    /* query ids (RowBlock::qid) */
  DMLC_AMD_LABEL = 5,  /* csv only: labels (rows carry labels only with label_column) */
  DMLC_AMD_FIELD = 6,  /* libfm only: field ids (RowBlock::field) */
  DMLC_AMD_NSLOT = 7
};

/* error codes in dmlc_amd_result.error & 0xFFFF (the first error by position) */
enum {
  DMLC_AMD_OK = 0,
  DMLC_AMD_ERR_NEG_INDEX = 1,   /* strtonum.h:416  CHECK_EQ(sign, true) */
  DMLC_AMD_ERR_NAN_LITERAL = 2, /* strtonum.h:163  "Invalid NAN literal" */
  DMLC_AMD_ERR_CSV_DELIM = 3,   /* csv_parser.h:128-132 delimiter not found */
  DMLC_AMD_ERR_CAPACITY = 16,   /* an output array was too small; counts are exact */
  DMLC_AMD_ERR_ARG = 32,        /* invalid argument (returned by the call itself) */
  DMLC_AMD_ERR_HIP = 33         /* HIP runtime error (returned by the call itself) */
};

typedef struct dmlc_amd_params {
  int32_t format;        /* DMLC_AMD_LIBSVM | CSV | LIBFM */
  int32_t index_bits;    /* 32 or 64: IndexType of dmlc::Parser<IndexType, DType> */
  int32_t value_type;    /* DMLC_AMD_F32 | I32 | I64: DType (csv only may be integral) */
  int32_t indexing_mode; /* libsvm/libfm: LibSVMParserParam::indexing_mode (libsvm_parser.h:32) */
  int32_t label_column;  /* csv: CSVParserParam::label_column, -1 = none (csv_parser.h:34) */
  int32_t weight_column; /* csv: CSVParserParam::weight_column, -1 = none (csv_parser.h:38) */
  int32_t delimiter;     /* csv: CSVParserParam::delimiter[0] (csv_parser.h:37) */
  uint32_t tile_bytes;   /* 0 = default tile size */
  uint32_t flags;        /* DMLC_AMD_FLAG_* */
  int32_t nthread;       /* FillData ranges per chunk (TextParserBase::nthread_, text_parser.h:32-35);
                            0 or 1 = one ParseBlock per chunk */
  uint32_t reserved[2];
} dmlc_amd_params;

#define DMLC_AMD_FLAG_COUNT_ONLY 1u /* run the counting passes only (size query) */
/* Run the write pass only, reusing the per-tile counts that a COUNT_ONLY call
 * on the same text, chunk starts, params and workspace left behind (earlier on
 * the same stream).  COUNT_ONLY then FILL_ONLY does exactly the work of one
 * full call, with a host-side allocation in between. */
#define DMLC_AMD_FLAG_FILL_ONLY 2u
/* Skip the single-pass uniform-grammar kernel and run the exact tile kernels
 * only (results are identical either way; this exists for testing/profiling). */
#define DMLC_AMD_FLAG_EXACT 4u
/* After the write pass, reduce the written index (and libfm field) arrays to
 * their maxima in dmlc_amd_result.max_index / max_field (the NumCol of the
 * reference's BasicRowIter, basic_row_iter.h:46-48). */
#define DMLC_AMD_FLAG_MAX_INDEX 8u

typedef struct dmlc_amd_csr {
  uint64_t *offset; /* rows + 1 (global, rebased across chunks) */
  void *label;      /* rows x DType (float for libsvm/libfm) */
  float *weight;
  uint64_t *qid;
  void *field;      /* IndexType */
  void *index;      /* IndexType */
  void *value;      /* DType */
  uint64_t cap[8];  /* capacity in elements per slot (cap[ROWS] counts labels; offset needs +1) */
} dmlc_amd_csr;

typedef struct dmlc_amd_result {
  uint64_t count[8];  /* exact totals per slot, even when a capacity was exceeded */
  uint64_t error;     /* 0, or (byte position << 16) | error code of the first error */
  uint64_t path;      /* 0 = single-pass uniform-grammar kernel, else exact tile kernels
                         (bit 1: the single-pass kernel handed over mid-launch) */
  uint64_t max_index; /* with DMLC_AMD_FLAG_MAX_INDEX: largest index written (0 if none) --
                         RowBlockContainer::max_index, row_block.h:126-168 */
  uint64_t max_field; /* likewise for libfm field ids (max_field) */
  uint64_t reserved[4];
} dmlc_amd_result;

/* Bytes of device workspace dmlc_amd_parse needs for this input. */
size_t dmlc_amd_workspace_bytes(uint64_t nbytes, int nchunks, const dmlc_amd_params *prm);

/* Parse.  d_chunk_table (optional, may be NULL) receives (nchunks * T) x 8
 * uint64, T = max(nthread, 1): the exclusive counts (slots above) at each
 * unit start.  Returns DMLC_AMD_OK
 * or DMLC_AMD_ERR_ARG / DMLC_AMD_ERR_HIP; parse errors are reported through
 * d_result->error once the stream reaches the end of the pipeline. */
int dmlc_amd_parse(const void *d_text, uint64_t nbytes, const uint64_t *d_chunk_starts, int nchunks,
                   const dmlc_amd_params *prm, const dmlc_amd_csr *out, uint64_t *d_chunk_table,
                   void *d_workspace, size_t workspace_bytes, dmlc_amd_result *d_result,
                   void *stream);

/* Dense row batch from a parsed CSR: the rows [row_begin, row_begin +
 * max_rows) that the parse produced, as a row-major matrix of ncol columns and
 * leading dimension ld >= ncol (in elements) at d_out, element type = the
 * value type.  With rows = min(result.count[ROWS], csr.cap[ROWS]):
 *
 *   for r in row_begin .. min(rows, row_begin + max_rows) - 1:
 *     out[(r - row_begin) * ld + 0 .. ncol-1] = fill
 *     for k in offset[r] .. offset[r+1]-1, ascending:
 *       c = index[k]                            (compared as 64-bit)
 *       if c < ncol: out[(r - row_begin) * ld + c] = count[VALUE] == 0 ? 1 : value[k]
 *       else:        dropped += 1; first_dropped = min(first_dropped, k)
 *
 * A later entry of the same row and column overwrites an earlier one (the last
 * wins, deterministically).  No value array means 1 (RowBlock::get_value,
 * include/dmlc/data.h).  Values are copied bit for bit.  Elements between ncol
 * and ld, and rows of d_out past the parsed row count, are never written;
 * d_out is never read.  fill_bits is the fill's bit pattern (its low 32 bits
 * for the 4-byte types).  libfm's field array is ignored. */
typedef struct dmlc_amd_dense_params {
  int32_t index_bits; /* 32 | 64 */
  int32_t value_type; /* DMLC_AMD_F32 | I32 | I64 */
  uint64_t row_begin, max_rows, ncol, ld, fill_bits;
  uint32_t flags, reserved[3]; /* 0 */
} dmlc_amd_dense_params;

/* d_status: uint64_t[4] in device memory, set by the call itself */
enum {
  DMLC_AMD_DENSE_ROWS = 0,    /* rows written (0 with flag bits 0 / 1) */
  DMLC_AMD_DENSE_DROPPED = 1, /* entries dropped because index >= ncol */
  DMLC_AMD_DENSE_FIRST = 2,   /* smallest position k of a dropped entry, ~0 if none */
  DMLC_AMD_DENSE_FLAGS = 3    /* DMLC_AMD_DENSE_FLAG_* */
};
#define DMLC_AMD_DENSE_FLAG_ERROR 1u       /* result.error != 0: nothing is written */
#define DMLC_AMD_DENSE_FLAG_VALUE_COUNT 2u /* count[VALUE] is neither 0 nor count[INDEX] (GetBlock's
                                              CHECK, row_block.h:171-189): nothing is written */
#define DMLC_AMD_DENSE_FLAG_OFFSET_CAP 4u  /* an offset pointed past the index (or value) capacity: no
                                              element at or past it is read, such entries are skipped */
#define DMLC_AMD_DENSE_FLAG_ROW_TOO_LONG 8u /* a row of 2^32 - 1 or more entries: its tile of rows is not
                                               written, the matrix is not valid */

/* Asynchronous on `stream`, after the parse that fills *d_result; no host
 * synchronisation, allocation or device-wide barrier.  csr->cap bounds every
 * read.  Returns DMLC_AMD_ERR_ARG before any HIP call for a null pointer,
 * ncol == 0, ld < ncol, bad index_bits / value_type, d_out not aligned to its
 * element, or a window of more tiles than one launch holds (2^31 - 1; see
 * dmlc_amd_dense_geometry -- split the rows over several calls).  max_rows ==
 * 0 only sets d_status. */
int dmlc_amd_to_dense(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result,
                      const dmlc_amd_dense_params *prm, void *d_out, uint64_t *d_status, void *stream);

/* Tile geometry this library was built with: a workgroup owns S = min(ncol,
 * cells_per_tile) columns of R = min(rows_per_tile, cells_per_tile / S) rows
 * (either pointer may be NULL). */
int dmlc_amd_dense_geometry(uint32_t *cells_per_tile, uint32_t *rows_per_tile);

/* Row gather of a parsed CSR: rows ids[0 .. n_ids) of `src`, in that order,
 * as a new compact CSR in `dst` (a shuffle, a subsample, a split; the device
 * form of RowBlockContainer::Push(Row) row by row, src/data/row_block.h).  With
 * rows = min(src_result.count[ROWS], src.cap[ROWS]):
 *
 *   dst.offset[0] = 0
 *   for i in 0 .. n_ids-1:
 *     r = ids[i]                                   (unsigned, compared as 64-bit)
 *     if r >= rows: bad += 1; first_bad = min(first_bad, i); the row is empty,
 *                   its label / weight / qid bits are 0
 *     else: append index / value / field[src.offset[r] .. src.offset[r+1]) to dst,
 *           label / weight / qid[i] = src ...[r]
 *     dst.offset[i+1] = entries so far
 *
 * A per-row array (label, weight, qid) is there iff its count in
 * *d_src_result is non-zero and equals count[ROWS]; a per-entry array (value,
 * field) iff its count is non-zero (it then equals count[INDEX], or flag bit 1
 * is raised).  Arrays that are not there are neither read nor written and
 * their count in *d_dst_result is 0.  Everything moves as bit patterns; an id
 * may repeat.  As in dmlc_amd_csr, cap[ROWS] is the capacity of label (and
 * offset holds cap[ROWS] + 1 words); a null array pointer has capacity 0, and
 * a source element at or past its capacity reads as 0.
 *
 * *d_dst_result has the layout a parse leaves: count[] = exact totals, even
 * past a capacity; path = 0; error = 0, or (i << 16) | DMLC_AMD_ERR_CAPACITY
 * with i the first position of ids whose row or entries did not fit -- nothing
 * at or past a capacity is written; max_index / max_field = 0, or with
 * DMLC_AMD_FLAG_MAX_INDEX the maxima of the dst arrays as written.  `dst` and
 * *d_dst_result can go straight into dmlc_amd_to_dense or another gather.
 *
 * Source and destination arrays must not overlap (undefined; the same pointer
 * on both sides is refused). */
typedef struct dmlc_amd_gather_params {
  int32_t index_bits;  /* 32 | 64 */
  int32_t value_type;  /* DMLC_AMD_F32 | I32 | I64: width of value[] */
  int32_t label_type;  /* width of label[]: F32 for libsvm/libfm, the DType for csv */
  int32_t id_bits;     /* 32 | 64: element type of d_ids */
  uint32_t flags;      /* 0 | DMLC_AMD_FLAG_MAX_INDEX */
  uint32_t reserved[3];
} dmlc_amd_gather_params;

/* d_status: uint64_t[4] in device memory, set by the call itself */
enum {
  DMLC_AMD_GATHER_ROWS = 0,  /* rows written: min(n_ids, dst.cap[ROWS]) (0 with flag bits 0 / 1) */
  DMLC_AMD_GATHER_BAD = 1,   /* ids at or past the source's rows */
  DMLC_AMD_GATHER_FIRST = 2, /* smallest position i of such an id, ~0 if none */
  DMLC_AMD_GATHER_FLAGS = 3  /* DMLC_AMD_GATHER_FLAG_* */
};
#define DMLC_AMD_GATHER_FLAG_ERROR 1u      /* src_result.error != 0: nothing is written, the dst counts are 0
                                              and dst_result.error is the source's */
#define DMLC_AMD_GATHER_FLAG_COUNT 2u      /* count[VALUE] or count[FIELD] is neither 0 nor count[INDEX]
                                              (GetBlock's CHECK, row_block.h:171-189): nothing is written, the
                                              dst counts are 0, dst_result.error is DMLC_AMD_ERR_ARG unless
                                              bit 0 is set too */
#define DMLC_AMD_GATHER_FLAG_OFFSET_CAP 4u /* a source offset pointed past the index (value, field) capacity:
                                              it is clamped, no element at or past the capacity is read */
#define DMLC_AMD_GATHER_FLAG_CAPACITY 8u   /* a dst capacity was exceeded (dst_result.error says where) */

/* Bytes of device workspace a gather of n_ids rows needs. */
size_t dmlc_amd_gather_workspace_bytes(uint64_t n_ids);

/* Asynchronous on `stream`, after whatever fills *d_src_result; no host
 * synchronisation, allocation or device-wide barrier, and no workgroup waits
 * for another.  The capacities bound every read and write.  Returns
 * DMLC_AMD_ERR_ARG before any HIP call for a null pointer (d_ids may be NULL
 * when n_ids == 0), bad index_bits / value_type / label_type / id_bits, a
 * non-zero reserved word or an unknown flag, a workspace that is too small,
 * more tiles than one launch holds (2^31 - 1; see dmlc_amd_gather_geometry),
 * or a dst array (or result block) that is the src's.  n_ids == 0 sets
 * d_status, dst.offset[0] and the result block only. */
int dmlc_amd_gather_rows(const dmlc_amd_csr *src, const dmlc_amd_result *d_src_result, const void *d_ids,
                         uint64_t n_ids, const dmlc_amd_gather_params *prm, const dmlc_amd_csr *dst,
                         dmlc_amd_result *d_dst_result, uint64_t *d_status, void *d_workspace,
                         size_t workspace_bytes, void *stream);

/* Ids per tile (one workgroup) this library was built with (the pointer may be NULL). */
int dmlc_amd_gather_geometry(uint32_t *rows_per_tile);

/* CSC transpose of a parsed CSR: the entries of rows [row_begin, row_begin +
 * max_rows) by column, a stable counting sort (what SparsePage::GetTranspose
 * does on the host; the column view a tree or coordinate-descent learner
 * reads).  `csr` and *d_result are a parse's or a gather's, unchanged.  With
 * rows = min(result.count[ROWS], csr.cap[ROWS]) and r1 = min(rows, row_begin +
 * max_rows):
 *
 *   kept = dropped = 0; first = ~0
 *   for r in row_begin .. r1-1:
 *     for k in offset[r] .. offset[r+1]-1, ascending:   (offsets clamped to the index / value
 *       c = index[k]            (compared as 64-bit)     capacity: flag bit 2, as in to_dense)
 *       if c >= ncol: dropped += 1; first = min(first, k)
 *       else: append (row = r - row_begin, value[k], pos = k) to column c
 *   col_offset[c] = entries of columns < c, for c in 0 .. ncol      (col_offset[ncol] = kept)
 *
 * The entries of a column stand in ascending source position k: ascending
 * row, duplicates of one cell in file order.  This is the only order the call
 * produces; two runs give the same bytes.  `value` (elements of the value type,
 * moved as bit patterns) is neither read nor written when count[VALUE] == 0 or
 * csc.value is NULL.  `pos`, when not NULL, receives each output entry's
 * absolute source position k, so anything else that is per entry (libfm's
 * field) follows by one index_select; the field array itself is ignored.  `cap`
 * bounds row, value and pos in entries: with kept > cap nothing at or past cap
 * is written, col_offset and the status stay exact and flag bit 3 is set.  All
 * ncol + 1 words of col_offset are written whatever the input.  max_rows == 0
 * or row_begin >= rows gives an empty CSC (col_offset all 0, kept = 0).  The
 * offsets of a parse or a gather never descend; for other offsets no access
 * leaves the capacities and the content is unspecified. */
typedef struct dmlc_amd_csc {
  uint64_t *col_offset; /* ncol + 1 words */
  uint32_t *row;        /* cap */
  void *value;          /* cap elements of the value type, or NULL */
  uint64_t *pos;        /* cap, or NULL */
  uint64_t cap;
} dmlc_amd_csc;

typedef struct dmlc_amd_csc_params {
  int32_t index_bits; /* 32 | 64 */
  int32_t value_type; /* DMLC_AMD_F32 | I32 | I64: width of value[] */
  uint64_t row_begin, max_rows;
  uint64_t ncol;        /* 1 .. 2^32 */
  uint64_t max_entries; /* the caller's bound on the window's entries: the launches and the workspace are
                           sized by it; 0 = csr.cap[INDEX] */
  uint32_t flags, reserved[3]; /* 0 */
} dmlc_amd_csc_params;

/* d_status: uint64_t[4] in device memory, set by the call itself */
enum {
  DMLC_AMD_CSC_KEPT = 0,    /* entries with index < ncol (exact, also past cap; 0 with flag bits 0 / 1) */
  DMLC_AMD_CSC_DROPPED = 1, /* entries dropped because index >= ncol */
  DMLC_AMD_CSC_FIRST = 2,   /* smallest position k of a dropped entry, ~0 if none */
  DMLC_AMD_CSC_FLAGS = 3    /* DMLC_AMD_CSC_FLAG_* (bits 0 - 2 as the dense and gather flags) */
};
#define DMLC_AMD_CSC_FLAG_ERROR 1u       /* result.error != 0: nothing is written but col_offset, all 0 */
#define DMLC_AMD_CSC_FLAG_VALUE_COUNT 2u /* count[VALUE] is neither 0 nor count[INDEX]: likewise */
#define DMLC_AMD_CSC_FLAG_OFFSET_CAP 4u  /* an offset pointed past the index (or value) capacity: it is
                                            clamped, no element at or past the capacity is read */
#define DMLC_AMD_CSC_FLAG_CAPACITY 8u    /* kept > csc.cap */
#define DMLC_AMD_CSC_FLAG_MAX_ENTRIES 16u /* the window holds more than max_entries entries: only its first
                                             max_entries were transposed (a caller's error) */

/* Bytes of device workspace a call with this bound on the window's entries
 * (not 0 here: pass csr.cap[INDEX] for the default) and these parameters
 * needs; 0 for parameters the call would refuse. */
size_t dmlc_amd_csc_workspace_bytes(uint64_t max_entries, uint64_t ncol, const dmlc_amd_csc_params *prm);

/* Asynchronous on `stream`, after whatever fills *d_result: a fixed sequence of
 * plain launches (three per 8-bit digit of ncol - 1, see dmlc_amd_csc_geometry),
 * no host synchronisation, allocation or device-wide barrier, and no workgroup
 * waits for another.  The capacities bound every read and write.  Returns
 * DMLC_AMD_ERR_ARG before any HIP call for a null pointer (csc.pos, and
 * csc.value when the caller has none, may be NULL), ncol == 0 or ncol > 2^32,
 * bad index_bits / value_type, a non-zero reserved word or an unknown flag, a
 * workspace that is too small, an output (or the workspace) that is one of the
 * source's arrays or its result block, or a window that can hold 2^32 - 1 or
 * more rows or entries (min(max_rows, cap[ROWS] - row_begin) rows, max_entries
 * entries: split the rows over several calls) -- which keeps `row` and the
 * internal positions at 32 bits. */
int dmlc_amd_to_csc(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_csc_params *prm,
                    const dmlc_amd_csc *csc, uint64_t *d_status, void *d_workspace, size_t workspace_bytes,
                    void *stream);

/* Entries per tile (one workgroup) and bits per digit pass this library was
 * built with (either pointer may be NULL). */
int dmlc_amd_csc_geometry(uint32_t *entries_per_tile, uint32_t *radix_bits);

/* Quantised dense row batch from a parsed CSR: what a histogram tree learner
 * trains on.  The rows [row_begin, row_begin + max_rows) that the parse
 * produced, as a row-major matrix of ncol columns and leading dimension ld >=
 * ncol (in elements) at d_out, each element the code_bytes-wide index of the
 * cell's bin under per-column cut points.  The window and the choice of each
 * cell's winning entry are dmlc_amd_to_dense's.  With rows =
 * min(result.count[ROWS], csr.cap[ROWS]):
 *
 *   for r in row_begin .. min(rows, row_begin + max_rows) - 1:
 *     win[0 .. ncol-1] = none
 *     for k in offset[r] .. offset[r+1]-1, ascending:
 *       c = index[k]                            (compared as 64-bit)
 *       if c < ncol: win[c] = count[VALUE] == 0 ? 1.0f : value[k]     (the last wins)
 *       else:        dropped += 1; first_dropped = min(first_dropped, k)
 *     for c in 0 .. ncol-1:
 *       code = missing_code
 *       if win[c] != none:
 *         v = win[c]; b = cut_ptr[c]; e = cut_ptr[c+1]; m = e - b
 *         if b > e or e > n_cuts: unbinned += 1; flags |= CUT_PTR
 *         else if m == 0:         unbinned += 1
 *         else if v is NaN:       nan += 1
 *         else:
 *           x = min(#{i in [b, e) : cut_value[i] <= v}, m - 1)       (IEEE compare)
 *           if flags & DMLC_AMD_BINS_GLOBAL: x += b
 *           if x fits code_bytes and x != missing_code: code = x
 *           else: flags |= CODE_RANGE
 *       out[(r - row_begin) * ld + c] = code
 *
 * x is the upper bound clamped to the last bin (XGBoost's
 * HistogramCuts::SearchBin; numpy's searchsorted(side="right") clipped to m -
 * 1): -0.0 == 0.0, -inf gives 0 and +inf gives m - 1.  cut_value is ascending
 * inside a column and holds no NaN; otherwise that column's codes are
 * unspecified (and still no access leaves the capacities).  No element of
 * cut_value at or past n_cuts is read.  Elements between ncol and ld, and rows
 * of d_out past the parsed row count, are never written; d_out is never read.
 * libfm's field array is ignored. */
typedef struct dmlc_amd_cuts { /* device arrays */
  const uint32_t *cut_ptr;     /* ncol + 1 words: column c owns cut_value[cut_ptr[c] .. cut_ptr[c+1]) */
  const float *cut_value;      /* n_cuts floats (may be NULL when n_cuts == 0) */
  uint64_t n_cuts;             /* capacity of cut_value: bounds every read */
} dmlc_amd_cuts;

#define DMLC_AMD_BINS_GLOBAL 1u /* codes are positions in cut_value: cut_ptr[c] is added */
typedef struct dmlc_amd_bins_params {
  int32_t index_bits;    /* 32 | 64 */
  int32_t value_type;    /* DMLC_AMD_F32 only */
  int32_t code_bytes;    /* 1 | 2 | 4: width of an output element */
  uint32_t missing_code; /* must fit code_bytes */
  uint64_t row_begin, max_rows, ncol, ld; /* as dmlc_amd_dense_params; ld in elements */
  uint32_t flags, reserved[3];            /* flags: DMLC_AMD_BINS_GLOBAL | 0 */
} dmlc_amd_bins_params;

/* d_status: uint64_t[8] in device memory, set by the call itself.  Words 0 - 3
 * are DMLC_AMD_DENSE_ROWS / DROPPED / FIRST / FLAGS with the dense flag bits 0 -
 * 3 (with bits 0 or 1 nothing is written to d_out); words 6 and 7 are 0. */
enum {
  DMLC_AMD_BINS_NAN = 4,     /* cells whose winning value was NaN */
  DMLC_AMD_BINS_UNBINNED = 5 /* cells with an entry in a column with no usable cuts */
};
#define DMLC_AMD_BINS_FLAG_CODE_RANGE 16u /* a code did not fit code_bytes or equalled missing_code: stored as
                                             missing_code */
#define DMLC_AMD_BINS_FLAG_CUT_PTR 32u    /* a cell's column has cut_ptr[c] > cut_ptr[c+1] or cut_ptr[c+1] > n_cuts */

/* Asynchronous on `stream`, after whatever fills *d_result; no host
 * synchronisation, allocation or device-wide barrier, and no workgroup waits
 * for another.  Returns DMLC_AMD_ERR_ARG before any HIP call for a null
 * pointer, ncol == 0 or ncol >= 2^32, ld < ncol, bad index_bits / value_type
 * (integer values are not binned) / code_bytes, a missing_code that does not
 * fit code_bytes, an unknown flag or a non-zero reserved word, d_out not
 * aligned to its element, d_out or d_status being one of the source's arrays,
 * its result block or a cut array, or a window of more tiles than one launch
 * holds (2^31 - 1; see dmlc_amd_bins_geometry).  max_rows == 0 only sets
 * d_status. */
int dmlc_amd_to_bins(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_cuts *cuts,
                     const dmlc_amd_bins_params *prm, void *d_out, uint64_t *d_status /* [8] */, void *stream);

/* Tile geometry, as dmlc_amd_dense_geometry (either pointer may be NULL). */
int dmlc_amd_bins_geometry(uint32_t *cells_per_tile, uint32_t *rows_per_tile);

/* Per-column quantile cut points from a parsed CSR: the cuts dmlc_amd_to_bins
 * quantises under, so parse -> (gather_rows) -> make_cuts -> to_bins runs on
 * one stream with no host round trip.  Exact rank quantiles over the entries
 * present in rows [row_begin, row_begin + max_rows), deduplicated (a column with
 * few distinct values gets few cuts); a column's last cut lies just above its
 * maximum.  `csr` and *d_result are a parse's or a gather's, unchanged.  The row
 * window, the clamping of offsets to the index / value capacity and the dropped
 * entries are dmlc_amd_to_csc's: an entry is dropped when index >= ncol
 * (compared as 64-bit).  Every other entry of the window is a sample of its
 * column, duplicates of one cell each counted; without a value array
 * (count[VALUE] == 0) every sample is 1.0f.
 *
 * All ordering is on an unsigned 32-bit key of the float's bits b; there is no
 * float compare and no float arithmetic, so the results are bit-exact:
 *
 *   if b == 0x80000000: b = 0                            (-0.0 counts as +0.0)
 *   if (b & 0x7fffffff) > 0x7f800000: key = 0xffffffff   (any NaN: sorts last, is no sample)
 *   else key = (b >> 31) ? ~b : b | 0x80000000
 *   unkey(k) = (k >> 31) ? k & 0x7fffffff : ~k
 *
 *   n_cuts = nan = empty = 0
 *   for c in 0 .. ncol-1:
 *     cut_ptr[c] = n_cuts
 *     s[0 .. n) = the ascending keys of column c's non-NaN samples; nan += its NaN samples
 *     if n == 0: empty += 1; continue       (to_bins counts the column's cells as UNBINNED)
 *     B = max_bin;  t[i] = s[floor(i * n / B)] for i in 0 .. B-1        (64-bit product)
 *     for i in 1 .. B-1: if t[i] > t[i-1]: emit unkey(t[i])             (every cut is > the minimum)
 *     top = s[n-1];  last = top == 0xff800000 (+inf) ? top : top + 1
 *     emit unkey(last), bits 0x80000000 stored as 0x00000000
 *   cut_ptr[ncol] = n_cuts
 *   (emit v: if n_cuts < out.cap: cut_value[n_cuts] = v;  n_cuts += 1)
 *
 * Under to_bins's code min(#{cuts <= v}, m - 1), N distinct values with max_bin
 * dividing N fall N / max_bin to a bin.  All ncol + 1 words of cut_ptr are
 * written whatever the input; an empty window gives all zeros.  With n_cuts >
 * out.cap no element of cut_value at or past cap is written, cut_ptr and the
 * status stay exact and flag bit 3 is set.  The outputs are a dmlc_amd_cuts
 * {cut_ptr, cut_value, n_cuts = out.cap} for dmlc_amd_to_bins, which never
 * reads past what cut_ptr names.  Two runs give the same bytes. */
typedef struct dmlc_amd_cuts_out {
  uint32_t *cut_ptr; /* ncol + 1 words */
  float *cut_value;  /* cap floats (may be NULL when cap == 0) */
  uint64_t cap;
} dmlc_amd_cuts_out;

typedef struct dmlc_amd_make_cuts_params {
  int32_t index_bits; /* 32 | 64 */
  int32_t value_type; /* DMLC_AMD_F32 only */
  uint64_t row_begin, max_rows, ncol, max_entries; /* as dmlc_amd_csc_params; max_entries 0 = csr.cap[INDEX] */
  uint32_t max_bin;            /* >= 1; ncol * max_bin < 2^32 */
  uint32_t flags, reserved[2]; /* 0 */
} dmlc_amd_make_cuts_params;

/* d_status: uint64_t[8] in device memory, set by the call itself.  Words 0 - 3
 * are DMLC_AMD_CSC_KEPT / DROPPED / FIRST / FLAGS (KEPT includes the NaN
 * samples); the flag bits are DMLC_AMD_CSC_FLAG_*: with ERROR or VALUE_COUNT
 * cut_ptr is all 0, N_CUTS is 0 and cut_value is untouched; CAPACITY means
 * N_CUTS > out.cap; MAX_ENTRIES that only the window's first max_entries
 * entries were sampled.  Word 7 is 0. */
enum {
  DMLC_AMD_CUTS_NAN = 4,       /* samples left out as NaN */
  DMLC_AMD_CUTS_N_CUTS = 5,    /* == cut_ptr[ncol] (exact, also past out.cap) */
  DMLC_AMD_CUTS_EMPTY_COLS = 6 /* columns with no cut */
};

/* Bytes of device workspace a call with this bound on the window's entries
 * (not 0 here: pass csr.cap[INDEX] for the default) and these parameters
 * needs; 0 for parameters the call would refuse. */
size_t dmlc_amd_make_cuts_workspace_bytes(uint64_t max_entries, uint64_t ncol, const dmlc_amd_make_cuts_params *prm);

/* Asynchronous on `stream`, after whatever fills *d_result: a fixed sequence of
 * plain launches sized by max_entries and ncol (three per 8-bit digit of the
 * key and of ncol - 1, then four more; see dmlc_amd_make_cuts_geometry), no
 * host synchronisation, allocation or device-wide barrier, and no workgroup
 * waits for another.  The capacities bound every read and write.  Returns
 * DMLC_AMD_ERR_ARG before any HIP call for a null pointer (out.cut_value may be
 * NULL when out.cap == 0), ncol == 0, max_bin == 0, ncol * max_bin >= 2^32
 * (which keeps cut_ptr at 32 bits), bad index_bits, a value_type other than
 * F32, a non-zero reserved word or an unknown flag, a workspace that is too
 * small, an output, the status or the workspace being one of the source's
 * arrays or its result block, or a window that can hold 2^32 - 1 or more rows
 * or entries (min(max_rows, cap[ROWS] - row_begin) rows, max_entries entries:
 * split the rows over several calls). */
int dmlc_amd_make_cuts(const dmlc_amd_csr *csr, const dmlc_amd_result *d_result, const dmlc_amd_make_cuts_params *prm,
                       const dmlc_amd_cuts_out *out, uint64_t *d_status /* [8] */, void *d_workspace,
                       size_t workspace_bytes, void *stream);

/* Entries per tile (one workgroup) and bits per digit pass this library was
 * built with (either pointer may be NULL). */
int dmlc_amd_make_cuts_geometry(uint32_t *entries_per_tile, uint32_t *radix_bits);

/* Batch dmlc::strtof (ParseFloat<float>, strtonum.h:95-264, :279-281): string i
 * is d_text[d_offsets[i] .. d_offsets[i+1]) read as NUL-terminated at its end.
 * Writes the value, the bytes consumed (endptr - nptr) and the "Invalid NAN
 * literal" flag (strtonum.h:163); d_consumed / d_nan_error may be NULL. */
int dmlc_amd_strtof_batch(const void *d_text, const uint64_t *d_offsets, uint64_t n, float *d_out,
                          uint32_t *d_consumed, uint32_t *d_nan_error, void *stream);

/* Stream copy of `bytes` between page-locked host memory (hipHostMalloc) and
 * device memory, or device to device, by a kernel instead of the DMA engine
 * (the host side of a parse pipeline: text batches in, CSR arrays out).  Both
 * pointers must be device-accessible; unaligned pointers fall back to
 * hipMemcpyAsync.  Asynchronous on `stream`. */
int dmlc_amd_copy(void *dst, const void *src, uint64_t bytes, void *stream);

/* n <= DMLC_AMD_COPY_MAX such copies (dst[i] <- src[i], bytes[i]) in one
 * kernel launch: the CSR arrays of a parsed batch in one D2H step.  Zero-byte
 * entries are skipped; a pair not 16-byte aligned is copied on its own. */
#define DMLC_AMD_COPY_MAX 16
int dmlc_amd_copy_n(void *const *dst, const void *const *src, const uint64_t *bytes, int n, void *stream);

/* The same with sizes known only on the device (a parse's result counts, so
 * the copy-out needs no host round trip after the parse): copy i moves
 * min(max_bytes[i], d_counts[slot[i]] * scale[i] + add[i]) bytes, or add[i]
 * when slot[i] < 0.  d_counts is read on the device when the copy runs: it
 * holds DMLC_AMD_COPY_SLOTS words (dmlc_amd_result.count), so slot[i] >=
 * DMLC_AMD_COPY_SLOTS is rejected (DMLC_AMD_ERR_ARG); slot / scale / add /
 * max_bytes are host arrays of n entries.  All pairs must be 16-byte
 * aligned. */
#define DMLC_AMD_COPY_SLOTS 8
int dmlc_amd_copy_n_dev(void *const *dst, const void *const *src, const uint64_t *d_counts, const int *slot,
                        const uint64_t *scale, const uint64_t *add, const uint64_t *max_bytes, int n,
                        void *stream);

/* Kernel timing for benchmarks: between profile_begin and profile_end, every
 * dmlc_amd_parse on this thread brackets its dominant kernel (the single-pass
 * kernel, or the exact write kernel) with HIP events on its stream.
 * profile_end synchronises, returns the summed kernel time, the number of
 * bracketed launches and the kernel's name. */
int dmlc_amd_profile_begin(void);
int dmlc_amd_profile_end(double *total_ms, int *launches, const char **kernel);

/* Human-readable message for an error code (matches the reference's CHECK text). */
const char *dmlc_amd_error_string(int code);

/* hipGetErrorString of the HIP error behind this thread's last DMLC_AMD_ERR_HIP. */
const char *dmlc_amd_last_hip_error(void);

/* Number of visible HIP devices (0 when no GPU / no driver). */
int dmlc_amd_device_count(void);

/* ABI version this library was built with. */
int dmlc_amd_abi_version(void);

/* Build id: SHA-256 (first 16 hex digits) of the kernel and C-ABI sources
 * this library was compiled from (dmlc-core_amd/Makefile).  bench.py stamps
 * its line with it and with the build id of the PMC run its HBM traffic
 * figure came from (profiles/traffic.json).  Not a reference interface. */
const char *dmlc_amd_build_id(void);

/* Geometry of the single-pass kernels this library was built with: text
 * bytes per tile and the most ParseBlock unit starts one tile takes before
 * the call goes to the exact kernels (diagnostics and tests; either pointer
 * may be NULL). */
int dmlc_amd_fast_geometry(uint32_t *tile_bytes, uint32_t *max_unit_starts);

#ifdef __cplusplus
}
#endif
#endif /* DMLC_AMD_H_ */
