// cuts.hip -- dmlc_amd_make_cuts: per-column quantile cut points of a parsed
// CSR's row window.  A stable LSD radix sort of the window's kept entries by
// (column, key of the float's bits), then rank picks per column (the tile
// bodies and their phases: cuts_core.h).  The source's counts are read on the
// device from its result block, so the call follows the parse, or a gather, on
// the same stream with no host round trip, and dmlc_amd_to_bins follows it.
// Three plain launches per 8-bit digit pass (hist, scan, scatter), then bounds,
// count, ptr and write.  No workgroup waits for another.
#include "block.h"
#include "cuts_core.h"
#include "dmlc_amd_kernels.h"

namespace dmlc_amd {
namespace {

using CutsBlock = DevBlockT<sizeof(CutsSum), kWaves>;
constexpr int kCutsScratchU64 = (int)(sizeof(CutsSum) / 8) * (kWaves + 1);

template <typename IT>
__global__ void __launch_bounds__(kThreads) cuts_hist_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  __shared__ uint32_t cnt[kCutsDigits];
  CutsBlock bk{scratch};
  cuts_hist_tile<IT>(a, blockIdx.x, cnt, bk);
}

__global__ void __launch_bounds__(kThreads) cuts_scan_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  CutsBlock bk{scratch};
  cuts_scan(a, blockIdx.x, bk);
}

template <typename IT, bool kFirst>
__global__ void __launch_bounds__(kThreads) cuts_scatter_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  __shared__ uint32_t cnt[kWaves * kCutsDigits];
  __shared__ uint32_t stage[2 * kCutsTile];
  __shared__ uint32_t gdelta[kCutsDigits + 1];
  CutsBlock bk{scratch};
  cuts_scatter_tile<IT, kFirst>(a, blockIdx.x, cnt, stage, gdelta, bk);
}

__global__ void __launch_bounds__(kThreads) cuts_bounds_kernel(const CutsArgs a) {
  cuts_bounds(a, (uint64_t)blockIdx.x * kThreads + threadIdx.x);
}

__global__ void __launch_bounds__(kThreads) cuts_count_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  CutsBlock bk{scratch};
  for (uint64_t c = blockIdx.x; c < a.ncol; c += gridDim.x) cuts_count_col(a, c, bk);
}

__global__ void __launch_bounds__(kThreads) cuts_ptr_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  CutsBlock bk{scratch};
  cuts_ptr(a, bk);
}

__global__ void __launch_bounds__(kThreads) cuts_write_kernel(const CutsArgs a) {
  __shared__ uint64_t scratch[kCutsScratchU64];
  CutsBlock bk{scratch};
  for (uint64_t c = blockIdx.x; c < a.ncol; c += gridDim.x) cuts_write_col(a, c, bk);
}

}  // namespace

hipError_t launch_make_cuts(const MakeCutsArgs &args, int wide, hipStream_t s) {
  CutsArgs a = args;
  const unsigned ntiles = (unsigned)a.ntiles;
  hipError_t e = hipSuccess;
  for (a.pass = 0; a.pass < a.passes; ++a.pass) {
    if (wide) cuts_hist_kernel<uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else cuts_hist_kernel<uint32_t><<<ntiles, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    cuts_scan_kernel<<<kCutsDigits, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (a.pass != 0) cuts_scatter_kernel<uint32_t, false><<<ntiles, kThreads, 0, s>>>(a);
    else if (wide) cuts_scatter_kernel<uint64_t, true><<<ntiles, kThreads, 0, s>>>(a);
    else cuts_scatter_kernel<uint32_t, true><<<ntiles, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  a.pass = a.passes;
  const unsigned nb = (unsigned)(a.ncol / kThreads + 1);  // ncol + 1 words
  const unsigned ng = (unsigned)mn<uint64_t>(a.ncol, kCutsMaxGrid);
  cuts_bounds_kernel<<<nb, kThreads, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  cuts_count_kernel<<<ng, kThreads, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  cuts_ptr_kernel<<<1, kThreads, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  cuts_write_kernel<<<ng, kThreads, 0, s>>>(a);
  return hipGetLastError();
}

}  // namespace dmlc_amd
