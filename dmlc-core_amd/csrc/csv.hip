// csv.hip -- MI355X kernels for CSVParser<I,D>::ParseBlock (csv_parser.h:71-149);
// the tile body lives in csv_core.h.
#include "block.h"
#include "csv_core.h"
#include "csv_fast.h"
#include "dmlc_amd_kernels.h"
#include "scan.h"

namespace dmlc_amd {
namespace {

template <int MODE>
#ifndef FEX_MINW
#define FEX_MINW 4  // waves per SIMD the exact tile kernels are register-budgeted for (round 4: 1 -> 4, config 3 exact 15.0 -> 13.6 ms; 5 waves spill more and lose: 14.9 ms)
#endif
__global__ void __launch_bounds__(kThreads, FEX_MINW) csv_tile(CsvArgs a) {
  __shared__ __attribute__((aligned(16))) csv::Shared sh;
  __shared__ uint64_t scratch[kBlockScratchU64];
  DevBlock bk{scratch};
  csv::tile<MODE>(a, sh, bk, blockIdx.x);
}

static_assert(sizeof(fcsv::Shared) + kSmallScratchU64 * 8 <= fast::kLdsBudget,
              "csv_fast_tile LDS above the 6-workgroup budget (fast_common.h kLdsBudget)");

#ifndef FCSV_MINW
#define FCSV_MINW 6
#endif
// the single-pass kernels (csv_fast.h tile<MODE, SP, VT, WS>), one launch
// bound and LDS for all: SP with a label and / or weight column, VT 1 the
// integer DTypes (strtoll), WS the whitespace mode (delimiter ' ' or '\t',
// FastCsvArgs::ws)
#define FCSV_KERNEL(NAME, SP, VT, WS)                                                       \
  template <int MODE>                                                                       \
  __global__ void __launch_bounds__(fast::kFThreads, FCSV_MINW) NAME(FastCsvArgs a) {       \
    __shared__ __attribute__((aligned(16))) fcsv::Shared sh;                                \
    __shared__ uint64_t scratch[kSmallScratchU64];                                          \
    DevBlockS bk{scratch};                                                                  \
    fcsv::tile<MODE, SP, VT, WS>(a, sh, bk, blockIdx.x);                                    \
  }
FCSV_KERNEL(csv_fast_tile, false, 0, false)
FCSV_KERNEL(csv_fast_tile_int, false, 1, false)
FCSV_KERNEL(csv_fast_tile_sp, true, 0, false)
FCSV_KERNEL(csv_fast_tile_ws, false, 0, true)
FCSV_KERNEL(csv_fast_tile_int_ws, false, 1, true)
FCSV_KERNEL(csv_fast_tile_sp_ws, true, 0, true)
FCSV_KERNEL(csv_fast_tile_int_sp, true, 1, false)
FCSV_KERNEL(csv_fast_tile_int_sp_ws, true, 1, true)
#undef FCSV_KERNEL

// the single-pass kernel of a call: by DType, label / weight columns and
// delimiter kind; the profile marks carry the name of the kernel that ran
template <int MODE>
void launch_fast_tile(const FastCsvArgs &f, bool sp, hipStream_t s) {
  const bool iv = f.vtype != 0, ws = f.ws != 0;
  const dim3 g(f.ntiles), b(fast::kFThreads);
#define FCSV_GO(NAME)                                           \
  do {                                                          \
    const char *nm = MODE == 1 ? #NAME "<1>" : #NAME "<2>";     \
    prof_mark(0, s, nm);                                        \
    NAME<MODE><<<g, b, 0, s>>>(f);                              \
    prof_mark(1, s, nm);                                        \
    return;                                                     \
  } while (0)
  if (ws) {
    if (iv && sp) FCSV_GO(csv_fast_tile_int_sp_ws);
    if (iv) FCSV_GO(csv_fast_tile_int_ws);
    if (sp) FCSV_GO(csv_fast_tile_sp_ws);
    FCSV_GO(csv_fast_tile_ws);
  }
  if (iv && sp) FCSV_GO(csv_fast_tile_int_sp);
  if (iv) FCSV_GO(csv_fast_tile_int);
  if (sp) FCSV_GO(csv_fast_tile_sp);
  FCSV_GO(csv_fast_tile);
#undef FCSV_GO
}

// label / weight columns: the single pass assumed one label (weight) entry per
// row (and, for label column 0, a delimiter in every row); a nonzero check sum
// hands the input to the exact kernels
__global__ void label_check_kernel(const uint64_t *labsum, uint32_t *gate) {
  const uint32_t i = threadIdx.x;  // kLabShards threads, one wave
  uint64_t a = labsum[i * 8], b = labsum[i * 8 + 1], c = labsum[i * 8 + 2];
  for (int d = 32; d >= 1; d >>= 1) {
    a += __shfl_xor(a, d, kWave);
    b += __shfl_xor(b, d, kWave);
    c += __shfl_xor(c, d, kWave);
  }
  if (i == 0 && (a != 0 || b != 0 || c != 0)) *gate |= 1u;
}

}  // namespace

hipError_t launch_csv(const CsvArgs &a, const FastCsvArgs &f, bool use_fast, uint64_t *res, int phase,
                      hipStream_t s) {
  hipError_t e;
  uint32_t *gate = f.gate;
  // ---- set-up, one launch (libsvm.hip launch_libsvm)
  FillList fl{};
  if (phase != kPhaseFill) {
    fill_result(fl, res);
    fl.gate = gate;
    fl.gate_v = use_fast ? 0u : 1u;
  }
  if (phase != kPhaseCount) fl.add(f.chunk_tab, (uint64_t)f.nchunk * 8, ~0ull);  // rows no tile writes: finish kernel
  fl.add(reinterpret_cast<uint64_t *>(f.err), 1, ~0ull);
  const bool sp = f.label_col >= 0 || f.weight_col >= 0;
  if (use_fast) {
    fl.add(f.lb, (uint64_t)f.ntiles * kCsvLbWords, 0);
    if (sp) fl.add(f.labsum, kLabShards * 8, 0);
  }
  if (!a.ntiles && phase != kPhaseCount) fl.add(reinterpret_cast<uint64_t *>(a.offset), 1, 0);  // empty input: offset = {0}
  if ((e = launch_prologue(fl, s)) != hipSuccess) return e;
  if (use_fast) {
    if (phase == kPhaseCount) launch_fast_tile<1>(f, sp, s);
    else launch_fast_tile<2>(f, sp, s);
    if (sp) label_check_kernel<<<1, kLabShards, 0, s>>>(f.labsum, gate);
  }
  launch_exact_tail(csv_tile<1>, csv_tile<2>, a, a, f.chunk_tab, f.nchunk, res, gate, phase, use_fast, "csv_tile<2>", s);
  finish_kernel<<<1, 256, 0, s>>>(res, gate, f.err, phase != kPhaseCount ? f.chunk_tab : nullptr, f.nchunk);
  return hipGetLastError();
}

}  // namespace dmlc_amd
