// libfm.hip -- MI355X kernels for LibFMParser<I>::ParseBlock (libfm_parser.h:67-144).
//   fm_fast_tile  single-pass uniform-grammar kernel (svm_fast.h with the
//                 libfm roles): the normal path; sets the gate word when the
//                 input leaves the grammar
//   libfm_tile    exact count / write tile kernels (libfm_core.h), run only
//                 when the gate is set (or indexing_mode < 0)
#include "block.h"
#include "dmlc_amd_kernels.h"
#include "libfm_core.h"
#include "scan.h"
#include "svm_fast.h"

namespace dmlc_amd {
namespace {

template <int MODE>
#ifndef FEX_MINW
#define FEX_MINW 5  // waves per SIMD the exact tile kernels are register-budgeted for (round 4: 1 -> 4, libfm 1M x 64 exact 22.4 -> 19.7 ms; round 6, with the role masks and records: 4 / 5 / 6 -> 7.15 / 6.74 / 7.76 ms, profiles/r6_ab/ab_exact_minw.txt)
#endif
__global__ void __launch_bounds__(kThreads, FEX_MINW) libfm_tile(LibfmArgs a) {
  __shared__ __attribute__((aligned(16))) svm::Shared sh;
  __shared__ uint64_t scratch[kBlockScratchU64];
  DevBlock bk{scratch};
  fm::tile<MODE>(a, sh, bk, blockIdx.x);
}

static_assert(sizeof(fsvm::Shared) + kSmallScratchU64 * 8 <= fast::kLdsBudget,
              "fm_fast_tile LDS above the 6-workgroup budget (fast_common.h kLdsBudget)");

#ifndef FFM_MINW
#define FFM_MINW (fast::kFWaves == 1 ? 5 : 6)
#endif
template <int MODE>
__global__ void __launch_bounds__(fast::kFThreads, FFM_MINW) fm_fast_tile(FastSvmArgs a) {
  __shared__ __attribute__((aligned(16))) fsvm::Shared sh;
  __shared__ uint64_t scratch[kSmallScratchU64];
  DevBlockS bk{scratch};
  fsvm::tile<MODE, true>(a, sh, bk, blockIdx.x);
}

}  // namespace

hipError_t launch_libfm(const LibfmArgs &a, const FastSvmArgs &f, bool use_fast, uint64_t *res, int phase,
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
  if (phase != kPhaseCount) fl.add(a.chunk_tab, (uint64_t)a.nchunk * 8, ~0ull);  // rows no tile writes: finish kernel
  fl.add(reinterpret_cast<uint64_t *>(f.err), 1, ~0ull);
  if (use_fast) {
    fl.add(f.lb, (uint64_t)f.ntiles * fast::kLbWords, 0);
    if (phase != kPhaseCount && f.indexing_mode < 0) fl.add(f.umin, (uint64_t)f.nchunk, ~0ull);
  }
  if (phase != kPhaseFill && a.indexing_mode < 0) fl.add(a.chunk_min, (uint64_t)a.nchunk, ~0ull);
  if (!a.ntiles && phase != kPhaseCount) fl.add(a.offset, 1, 0);  // empty input: offset = {0}
  if ((e = launch_prologue(fl, s)) != hipSuccess) return e;
  if (use_fast) {
    if (phase == kPhaseCount) {
      fm_fast_tile<1><<<f.ntiles, fast::kFThreads, 0, s>>>(f);  // (unmarked, unlike the other two formats' count phase)
    } else {
      prof_mark(0, s, "fm_fast_tile<2>");
      fm_fast_tile<2><<<f.ntiles, fast::kFThreads, 0, s>>>(f);
      prof_mark(1, s, "fm_fast_tile<2>");
    }
  }
  // (a.chunk_tab where the other two reset f.chunk_tab: never null -- the
  // workspace's table when the caller gives none)
  launch_exact_tail(libfm_tile<1>, libfm_tile<2>, a, a, a.chunk_tab, f.nchunk, res, gate, phase, use_fast,
                    "libfm_tile<2>", s);
  finish_kernel<<<1, 256, 0, s>>>(res, gate, f.err, phase != kPhaseCount ? a.chunk_tab : nullptr, a.nchunk);
  if (use_fast && phase != kPhaseCount && f.indexing_mode < 0 &&
      (e = launch_umin_fix(f.index, f.field, f.wide, f.chunk_tab, f.nchunk, f.umin, res, gate, f.cap[C_INDEX], f.cap[C_FIELD], s)) !=
          hipSuccess)
    return e;
  return hipGetLastError();
}

}  // namespace dmlc_amd
