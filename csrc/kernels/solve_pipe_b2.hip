// Pipelined matrix-core MU solve (solve_pipe.h): K = 17..24.
#include "solve_pipe.h"

namespace cnmf {
hipError_t launch_solve_pipe_b2(int K, const SolveParams& p, int nblocks, int T, int pl_n,
                                hipStream_t s) {
  return launch_pipe_ranks(K, rank_range<17, 24>{}, p, nblocks, T, pl_n, s);
}
}  // namespace cnmf
