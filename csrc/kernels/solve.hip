// Launcher + C ABI of the fused inner solve (kernels in solve_core.h).  This unit
// instantiates the streaming variant for K <= 32; solve_wide.hip the wide streaming ranks,
// solve_res.hip / solve_res34.hip the register-resident one, solve_mfma.hip,
// solve_wmfma.hip and solve_pipe*.hip the matrix-core bodies.
#include "launchers.h"
#include "solve_core.h"

namespace cnmf {
hipError_t launch_solve_stream(int K, int algo, const SolveParams& p, int nblocks, int threads,
                               hipStream_t s) {
  return launch_solve_stream_ranks(K, rank_range<1, 32>{}, algo, p, nblocks, threads, s);
}
}  // namespace cnmf

extern "C" int cnmf_solve_max_k() { return 128; }

// ranks the kernels are instantiated for: 1..32, the padded wide ranks 40..64 (multiples
// of 8) and 80..128 (multiples of 16, MU only: solve_wmfma.hip)
extern "C" int cnmf_solve_native_k(int K) {
  return (K >= 1 && K <= 32) || K == 40 || K == 48 || K == 56 || K == 64 || K == 80 ||
         K == 96 || K == 112 || K == 128;
}

extern "C" int cnmf_solve_max_threads(int K) { return K > 32 ? 256 : 1024; }

extern "C" int cnmf_solve_reg_max_cols(int K) {
  return K <= cnmf::kResidentMaxK ? 1024 * cnmf::res_max_cols(K) : 0;
}

extern "C" hipError_t cnmf_solve(int algo, int K, float* x, long long x_rs, long long ldx,
                                 const float* numer, long long n_rs, long long ldn,
                                 const float* gram, long long g_rs, const int* rep_index,
                                 int nblocks, int ncols, int max_iter, float tol, float l1_num,
                                 float l1_den, float l2, float eps, float* lin_out,
                                 float* quad_out, int* iters_out, int nsplit, int conv_mode,
                                 int check_every, int threads, int kernel,
                                 const int* active, int coop_split, float* coop_slots,
                                 unsigned coop_gen, int coop_epochs, int* coop_timeout,
                                 unsigned short* planes, long long pl_rs, long long pl_ld,
                                 long long pl_plane, const float* pl_colmul, int pl_cols,
                                 int pl_n, const float* gsrc, long long gs_rs, long long gs_ld,
                                 int gs_cols, int nslab_n, long long nslab_stride, const float* n_scale, const float* nbase,
                                 float* nout, long long nb_rs, long long ldnb, const float* gpart,
                                 int gpart_n, long long gpart_rs, float* gout, float* gp_out,
                                 long long gp_rs, unsigned* coop_gen_dev, unsigned* coop_arrive,
                                 int reps_per_launch, unsigned long long* stamps,
                                 hipStream_t stream) {
  if (nblocks <= 0) return hipSuccess;
  // buffer offsets are 32-bit: a replicate's block must span < 2 GiB
  if ((long long)K * (ldx > ldn ? ldx : ldn) * 4 >= 0x7fffffffLL) return hipErrorInvalidValue;
  cnmf::SolveParams p;
  p.x = x; p.x_rs = x_rs; p.ldx = ldx;
  p.numer = numer; p.n_rs = n_rs; p.ldn = ldn;
  p.gram = gram; p.g_rs = g_rs;
  p.rep_index = rep_index;
  p.rep0 = 0;
  p.ncols = ncols; p.max_iter = max_iter;
  p.tol = tol; p.l1_num = l1_num; p.l1_den = l1_den; p.l2 = l2; p.eps = eps;
  p.lin_out = lin_out; p.quad_out = quad_out; p.iters_out = iters_out;
  p.nsplit = nsplit;
  p.conv_mode = conv_mode;
  p.check_every = check_every;
  p.active = active;
  p.coop_slots = coop_split > 1 ? (unsigned long long*)coop_slots : nullptr;
  p.coop_gen = coop_gen;
  p.coop_epochs = coop_epochs;
  p.coop_timeout = coop_timeout;
  p.coop_epochs_split = coop_split > 1 ? coop_split : 1;
  p.planes = planes; p.pl_rs = pl_rs; p.pl_ld = pl_ld; p.pl_plane = pl_plane;
  p.pl_colmul = pl_colmul; p.pl_cols = pl_cols;
  p.pl_n = pl_n < 1 ? 1 : (pl_n > 3 ? 3 : pl_n);
  p.gsrc = gsrc; p.gs_rs = gs_rs; p.gs_ld = gs_ld; p.gs_cols = gs_cols;
  p.nslab_n = nslab_n < 1 ? 1 : nslab_n; p.nslab_stride = nslab_stride; p.n_scale = n_scale;
  p.nbase = nbase; p.nout = nout; p.nb_rs = nb_rs; p.ldnb = ldnb;
  p.gpart = gpart; p.gpart_n = gpart_n; p.gpart_rs = gpart_rs; p.gout = gout;
  p.gp_out = gp_out; p.gp_rs = gp_rs;
  p.coop_gen_dev = coop_split > 1 ? coop_gen_dev : nullptr;
  p.coop_arrive = coop_arrive;
  p.stamps = stamps;
  // workgroup order of the pipelined kernel (SolveParams.pipe_map); CNMF_PIPE_MAP
  // overrides the default for A/B runs
  static const int map_env = [] {
    const char* e = getenv("CNMF_PIPE_MAP");
    return (e && *e) ? atoi(e) : -1;
  }();
  p.pipe_map = map_env;     // < 0: chosen per launch below
  p.pipe_nblocks = nblocks;
  if (p.coop_gen_dev && !coop_arrive) return hipErrorInvalidValue;
  const bool fused = p.nslab_n > 1 || n_scale || nbase || nout || gpart || gout || gp_out ||
                     (coop_split > 1 && coop_gen_dev);
  if (fused && (p.nslab_n > 1 && p.nslab_stride * 4 * (long long)p.nslab_n >= 0x7fffffffLL))
    return hipErrorInvalidValue;
  if (planes && pl_cols < ncols) return hipErrorInvalidValue;
  if (coop_split > 1 && nsplit > 1) return hipErrorInvalidValue;
  if (coop_split > cnmf::kCoopMaxSlices) return hipErrorInvalidValue;
  if (!cnmf_solve_native_k(K)) return hipErrorInvalidValue;
  // `kernel` is the host planner's choice (ops.solve_plan; the rules are the table "Solve
  // dispatch" in docs/ARCHITECTURE.md).  Each case checks that kernel's own preconditions
  // -- a failed one is an error, never another kernel -- and derives only what follows from
  // its geometry (tiles, columns per thread, workgroup order).
  // columns per slice, by the kernels' own rule (solve_slice in solve_core.h)
  const int parts = nsplit > 1 ? nsplit : (coop_split > 1 ? coop_split : 1);
  const int per = cnmf::solve_cols_per_slice(ncols, parts);
  // the in-prologue Gram is solve_mfma's; fused operands and launch rounds (reps_per_launch
  // replicates at a time, each round co-resident) the pipelined kernel's: never dropped
  if (gsrc && (kernel != CNMF_SOLVE_mfma || gs_cols < 1)) return hipErrorInvalidValue;
  if (kernel != CNMF_SOLVE_pipe &&
      (fused || (!gram && !gsrc) || (reps_per_launch > 0 && reps_per_launch < nblocks)))
    return hipErrorInvalidValue;
  switch (kernel) {
    case CNMF_SOLVE_pipe: {   // solve_pipe.h: unregularised block-objective MU, K <= 64
      const int Tp = cnmf_solve_pipe_tiles(K, per);
      if (algo != 0 || Tp == 0 || conv_mode != 1 || nsplit > 1 || l1_num != 0.f ||
          l1_den != 0.f || l2 != 0.f || (!gram && !gpart))
        return hipErrorInvalidValue;
      const int rpl = reps_per_launch > 0 ? reps_per_launch : nblocks;
      if (p.pipe_map < 0) {
        // XCD-grouped slices (one L2 for a replicate's exchanges: the objective checks
        // cost ~half) when the launch runs in ONE round and each XCD's share fits its
        // resident budget.  Measured (profiles/r4za_*): headline 13,133-13,198 ->
        // 13,482-13,535 rep/s, K=5..13 grid 18,972 -> 19,677; launches in several rounds
        // (K = 20 / 30 usage side) lost with it (r4g, r4z), so they keep the plain order
        static int n_cu[16] = {0};
        int dev = 0, v = 0;
        (void)hipGetDevice(&dev);
        if (dev < 0 || dev >= 16) dev = 0;
        if (n_cu[dev] == 0)
          n_cu[dev] = hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) ==
                              hipSuccess && v > 0 ? v : 256;
        const int S = coop_split > 1 ? coop_split : 1;
        const long long per_xcd = (long long)cnmf_solve_pipe_wg_per_cu(K) * n_cu[dev] / 8;
        p.pipe_map = (S > 1 && rpl >= nblocks && (long long)((rpl + 7) / 8) * S <= per_xcd) ? 1 : 0;
      }
      for (int r0 = 0; r0 < nblocks; r0 += rpl) {
        p.rep0 = r0;
        const hipError_t e = cnmf::launch_solve_pipe(K, p, nblocks - r0 < rpl ? nblocks - r0 : rpl,
                                                     Tp, p.pl_n, stream);
        if (e != hipSuccess) return e;
      }
      return hipSuccess;
    }
    case CNMF_SOLVE_mfma: {   // solve_mfma.hip: MU, K <= 16, penalties, nsplit, in-prologue Gram
      if (algo != 0 || per > cnmf_solve_mfma_max_cols(K)) return hipErrorInvalidValue;
      const int T = ((per + 15) / 16 + 3) / 4;
      return cnmf::launch_solve_mfma(K, p, nblocks, T < 1 ? 1 : T, stream);
    }
    // K > 64: the matrix-core wide solve, MU only (HALS is Gauss-Seidel over components).
    // Split-bf16 Gram apply at K = 96 / 128 (whole 32-deep k-blocks); fp32 MFMA at 80 / 112:
    // padding those to 96 / 128 inside the kernel cost occupancy and measured slower
    // (profiles/r3af_*)
    case CNMF_SOLVE_wmfma_bf16:
    case CNMF_SOLVE_wmfma_f32: {
      const bool bf16 = kernel == CNMF_SOLVE_wmfma_bf16;
      if (algo != 0 || (bf16 && K % 32 != 0)) return hipErrorInvalidValue;
      return cnmf::launch_solve_wmfma(K, p, nblocks, bf16, stream);
    }
    case CNMF_SOLVE_wide:
      return cnmf::launch_solve_wide(K, algo, p, nblocks, threads, stream);
    case CNMF_SOLVE_resident: {
      // every slice must fit U <= res_max_cols(K) columns per thread of a <= 1024-thread
      // workgroup; it runs with the smallest such U and just enough threads for the slice
      const int U = per <= 1024 ? 1 : (per + 1023) / 1024;
      if (K > cnmf::kResidentMaxK || U > cnmf::res_max_cols(K)) return hipErrorInvalidValue;
      int t_res = (((per + U - 1) / U + 63) / 64) * 64;
      if (t_res < 64) t_res = 64;
      return cnmf::launch_solve_resident(K, U, algo, p, nblocks, t_res, stream);
    }
    case CNMF_SOLVE_stream:
      return cnmf::launch_solve_stream(K, algo, p, nblocks, threads, stream);
    default:
      return hipErrorInvalidValue;
  }
}
