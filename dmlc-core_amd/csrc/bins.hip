// bins.hip -- dmlc_amd_to_bins: a parsed batch's CSR, or a row window of it, as
// a dense row-major matrix of bin codes under per-column cut points (the tile
// body and its phases: bins_core.h).  As dense.hip: the row and entry counts
// are read on the device from the parse's result block, so the call follows
// dmlc_amd_parse (or a gather) on the same stream with no host round trip.
// Two launches: one thread sets d_status, then one workgroup per tile.
#include "bins_core.h"
#include "block.h"
#include "dmlc_amd_kernels.h"

namespace dmlc_amd {
namespace {

__global__ void __launch_bounds__(kWave) bins_status_kernel(const BinsArgs b) {
  if (threadIdx.x == 0) bins_status_init(b);
}

template <typename IT, typename CT>
__global__ void __launch_bounds__(kThreads) bins_tile_kernel(const BinsArgs b) {
  __shared__ __attribute__((aligned(16))) uint32_t tags[kDenseCells];
  __shared__ uint64_t offs[kDenseRows + 1];
  __shared__ uint32_t cptr[kDenseCells + 1];
  __shared__ float lcut[kBinsLdsCuts];
  __shared__ uint32_t sm[BL_WORDS];
  DevBlockT<8, kWaves> bk{nullptr};
  bins_tile<IT, CT>(b, blockIdx.x, tags, offs, cptr, lcut, sm, bk);
}

template <typename IT>
void launch_tiles(const BinsArgs &b, int code_bytes, uint32_t ntiles, hipStream_t s) {
  if (code_bytes == 1) bins_tile_kernel<IT, uint8_t><<<ntiles, kThreads, 0, s>>>(b);
  else if (code_bytes == 2) bins_tile_kernel<IT, uint16_t><<<ntiles, kThreads, 0, s>>>(b);
  else bins_tile_kernel<IT, uint32_t><<<ntiles, kThreads, 0, s>>>(b);
}

}  // namespace

hipError_t launch_bins(const BinsArgs &b, int wide, int code_bytes, uint32_t ntiles, hipStream_t s) {
  bins_status_kernel<<<1, kWave, 0, s>>>(b);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || ntiles == 0) return e;
  if (wide) launch_tiles<uint64_t>(b, code_bytes, ntiles, s);
  else launch_tiles<uint32_t>(b, code_bytes, ntiles, s);
  return hipGetLastError();
}

}  // namespace dmlc_amd
