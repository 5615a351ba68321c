// dense.hip -- dmlc_amd_to_dense: a parsed batch's CSR, or a row window of
// it, as a dense row-major matrix with a fill for missing cells (the tile body
// and its phases: dense_core.h).  The row and entry counts are read on the
// device from the parse's result block, so the call follows dmlc_amd_parse on
// the same stream with no host round trip; tiles past the parsed rows leave at
// once.  Two launches: one thread sets d_status, then one workgroup per tile.
#include "block.h"
#include "dense_core.h"
#include "dmlc_amd_kernels.h"

namespace dmlc_amd {
namespace {

__global__ void __launch_bounds__(kWave) dense_status_kernel(const DenseArgs a) {
  if (threadIdx.x == 0) dense_status_init(a);
}

template <typename IT, typename VT>
__global__ void __launch_bounds__(kThreads) dense_tile_kernel(const DenseArgs a) {
  __shared__ __attribute__((aligned(16))) uint32_t tags[kDenseCells];
  __shared__ uint64_t offs[kDenseRows + 1];
  __shared__ uint32_t bad;
  DevBlockT<8, kWaves> bk{nullptr};
  dense_tile<IT, VT>(a, blockIdx.x, tags, offs, &bad, bk);
}

}  // namespace

hipError_t launch_dense(const DenseArgs &a, int wide, int value_bytes, uint32_t ntiles, hipStream_t s) {
  dense_status_kernel<<<1, kWave, 0, s>>>(a);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess || ntiles == 0) return e;
  if (wide) {
    if (value_bytes == 8) dense_tile_kernel<uint64_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else dense_tile_kernel<uint64_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
  } else {
    if (value_bytes == 8) dense_tile_kernel<uint32_t, uint64_t><<<ntiles, kThreads, 0, s>>>(a);
    else dense_tile_kernel<uint32_t, uint32_t><<<ntiles, kThreads, 0, s>>>(a);
  }
  return hipGetLastError();
}

}  // namespace dmlc_amd
