// gather.hip -- dmlc_amd_gather_rows: rows ids[0 .. n_ids) of a parsed CSR as a
// new compact CSR (the tile bodies and their phases: gather_core.h).  The
// source's row and entry counts are read on the device from its result block,
// so the call follows the parse, or another gather, on the same stream with no
// host round trip.  Three plain launches: the tiles' entry counts, their scan
// by one workgroup (which also sets d_status and the dst result block), the
// copy.  No workgroup waits for another.
#include "block.h"
#include "gather_core.h"
#include "dmlc_amd_kernels.h"

namespace dmlc_amd {
namespace {

using GatherBlock = DevBlockT<sizeof(GatherRec), kWaves>;
constexpr int kGatherScratchU64 = (int)(sizeof(GatherRec) / 8) * (kWaves + 1);

__global__ void __launch_bounds__(kThreads) gather_lengths_kernel(const GatherArgs a) {
  __shared__ uint64_t scratch[kGatherScratchU64];
  GatherBlock bk{scratch};
  gather_lengths_tile(a, blockIdx.x, bk);
}

__global__ void __launch_bounds__(kThreads) gather_scan_kernel(const GatherArgs a) {
  __shared__ uint64_t scratch[kGatherScratchU64];
  GatherBlock bk{scratch};
  gather_scan(a, bk);
}

template <typename IT, typename VT>
__global__ void __launch_bounds__(kThreads) gather_copy_kernel(const GatherArgs a) {
  __shared__ uint64_t scratch[kGatherScratchU64];
  __shared__ uint64_t dpos[kGatherRows + 1];
  __shared__ uint64_t spos[kGatherRows];
  GatherBlock bk{scratch};
  gather_copy_tile<IT, VT>(a, blockIdx.x, dpos, spos, bk);
}

}  // namespace

hipError_t launch_gather(const GatherArgs &a, int wide, int value_bytes, hipStream_t s) {
  const unsigned ntiles = (unsigned)a.ntiles;
  hipError_t e = hipSuccess;
  if (ntiles) {
    gather_lengths_kernel<<<ntiles, kThreads, 0, s>>>(a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
  }
  gather_scan_kernel<<<1, kThreads, 0, s>>>(a);
  if ((e = hipGetLastError()) != hipSuccess || ntiles == 0) return e;
  if (wide) {
    if (value_bytes == 8) gather_copy_kernel<uint64_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else gather_copy_kernel<uint64_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
  } else {
    if (value_bytes == 8) gather_copy_kernel<uint32_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else gather_copy_kernel<uint32_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace dmlc_amd
