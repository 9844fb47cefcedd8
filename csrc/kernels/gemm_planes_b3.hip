// Split-precision GEMM, narrow tile variants for outputs of few rows (the tail layouts of
// an online batch): an instantiation unit of gemm_planes.h.
//   8 = 128 x 64 (4 waves of 64 x 32, NI = 2)
//   9 = 128 x 32 (4 waves of 64 x 16, NI = 1): a 100 x 5000 output is 157 tiles
// so a one-tile-high product fills most of the chip without a k split (no slabs to sum).
#include "gemm_planes.h"

namespace cnmf {

template <int PA, int PB>
static hipError_t launch_narrow(int v, const PlaneGemmParams& p, int stages, int bk,
                                hipStream_t s) {
  const bool deep = bk >= 64 && p.Kd % 64 == 0;
  if (v == 8)
    return deep ? launch_gemm<PA, PB, 64, 2, 2, 4, 2>(p, stages, s)
                : launch_gemm<PA, PB, 32, 2, 2, 4, 2>(p, stages, s);
  return deep ? launch_gemm<PA, PB, 64, 2, 2, 4, 1>(p, stages, s)
              : launch_gemm<PA, PB, 32, 2, 2, 4, 1>(p, stages, s);
}

hipError_t launch_gemm_narrow(int pa, int pb, int v, const PlaneGemmParams& p, int stages,
                              int bk, hipStream_t s) {
  CNMF_GEMM_DISPATCH_PLANES(launch_narrow, pa, pb, v, p, stages, bk, s)
}

}  // namespace cnmf
