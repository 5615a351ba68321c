// csc.hip -- dmlc_amd_to_csc: the CSC transpose of a parsed CSR's row window, a
// stable LSD radix sort of its entries by column (the tile bodies and their
// phases: csc_core.h).  The source's counts are read on the device from its
// result block, so the call follows the parse, or a gather, on the same stream
// with no host round trip.  Three plain launches per 8-bit digit pass (hist,
// scan, scatter), and one more for col_offset when there is more than one
// pass.  No workgroup waits for another.
#include "block.h"
#include "csc_core.h"
#include "dmlc_amd_kernels.h"

namespace dmlc_amd {
namespace {

using CscBlock = DevBlockT<sizeof(CscRec), kWaves>;
constexpr int kCscScratchU64 = (int)(sizeof(CscRec) / 8) * (kWaves + 1);

template <typename IT>
__global__ void __launch_bounds__(kThreads) csc_hist_kernel(const CscArgs a) {
  __shared__ uint64_t scratch[kCscScratchU64];
  __shared__ uint32_t cnt[kCscDigits];
  CscBlock bk{scratch};
  csc_hist_tile<IT>(a, blockIdx.x, cnt, bk);
}

__global__ void __launch_bounds__(kThreads) csc_scan_kernel(const CscArgs a) {
  __shared__ uint64_t scratch[kCscScratchU64];
  CscBlock bk{scratch};
  csc_scan(a, blockIdx.x, bk);
}

template <typename IT, typename VT>
__global__ void __launch_bounds__(kThreads) csc_scatter_kernel(const CscArgs a) {
  __shared__ uint64_t scratch[kCscScratchU64];
  __shared__ uint32_t cnt[kWaves * kCscDigits];
  __shared__ uint32_t span[kCscSpan + 1];
  __shared__ uint64_t ends[2];
  CscBlock bk{scratch};
  csc_scatter_tile<IT, VT>(a, blockIdx.x, cnt, span, ends, bk);
}

__global__ void __launch_bounds__(kThreads) csc_bounds_kernel(const CscArgs a) {
  csc_bounds(a, (uint64_t)blockIdx.x * kThreads + threadIdx.x);
}

}  // namespace

hipError_t launch_csc(const CscArgs &args, int wide, int value_bytes, hipStream_t s) {
  CscArgs a = args;
  const unsigned ntiles = (unsigned)a.ntiles;
  hipError_t e = hipSuccess;
  for (a.pass = 0; a.pass < a.passes; ++a.pass) {
    if (wide) csc_hist_kernel<uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else csc_hist_kernel<uint32_t><<<ntiles, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    csc_scan_kernel<<<kCscDigits, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (wide) {
      if (value_bytes == 8) csc_scatter_kernel<uint64_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
      else csc_scatter_kernel<uint64_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
    } else {
      if (value_bytes == 8) csc_scatter_kernel<uint32_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
      else csc_scatter_kernel<uint32_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
    }
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  if (a.passes > 1) {
    const unsigned nb = (unsigned)(a.ncol / kThreads + 1);  // ncol + 1 words
    csc_bounds_kernel<<<nb, kThreads, 0, s>>>(a);
    e = hipGetLastError();
  }
  return e;
}

}  // namespace dmlc_amd
