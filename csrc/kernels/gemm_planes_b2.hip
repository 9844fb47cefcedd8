// Split-precision GEMM, tile variants with five 16-column blocks per wave (NI = 5): an
// instantiation unit of gemm_planes.h, apart from gemm_planes.hip to bound build time.
//   6 = 128 x 160 (4 waves of 64 x 80): a 1000 x 5000 output is 8 x 32 = 256 tiles
//   7 = 128 x 320 (8 waves of 64 x 80): a 2000 x 5000 output is 16 x 16 = 256 tiles
// i.e. one workgroup per CU in one wave of workgroups, with no k split.
#include "gemm_planes.h"

namespace cnmf {

template <int PA, int PB>
static hipError_t launch_wide(int v, const PlaneGemmParams& p, int stages, int bk,
                              hipStream_t s) {
  const bool deep = bk >= 64 && p.Kd % 64 == 0;
  if (v == 6)
    return deep ? launch_gemm<PA, PB, 64, 2, 2, 4, 5>(p, stages, s)
                : launch_gemm<PA, PB, 32, 2, 2, 4, 5>(p, stages, s);
  return deep ? launch_gemm<PA, PB, 64, 2, 4, 4, 5>(p, stages, s)
              : launch_gemm<PA, PB, 32, 2, 4, 4, 5>(p, stages, s);
}

hipError_t launch_gemm_wide(int pa, int pb, int v, const PlaneGemmParams& p, int stages, int bk,
                            hipStream_t s) {
  CNMF_GEMM_DISPATCH_PLANES(launch_wide, pa, pb, v, p, stages, bk, s)
}

}  // namespace cnmf
