// Shared pieces of the sparse KL kernels (sparse_kl.hip: K <= 32, sparse_kl_wide.hip:
// 33 <= K <= 64, sparse_kl_xwide.hip: 65 <= K <= 128): launch parameters, the DPP helper
// and the stopping-rule tail.
#pragma once
#include <hip/hip_runtime.h>

#include "common.h"

namespace cnmf {

typedef float sk_f2 __attribute__((ext_vector_type(2)));

constexpr int kSkThreads = 256;                 // global-gather variant
constexpr int kSkThreadsL = 512;                // LDS variant (one workgroup per CU)
constexpr int kSkRow = 16;                      // lanes per fixed column (one DPP row)
constexpr int kSkCols = kSkThreads / kSkRow;    // columns in flight per workgroup
constexpr int kSkLdsBytes = 128 * 1024;         // LDS budget for the staged S^T rows
constexpr int kSkMaxK = 32;                     // sk_kernel; above it sk_wide_kernel
constexpr int kSkWideMaxK = 64;                 // sk_wide_kernel; above it sk_xwide_kernel
constexpr int kSkXWideMaxK = 128;

struct SkParams {
  const int* rowptr;   // (Lf + 1): fixed column i owns entries [rowptr[i], rowptr[i+1])
  const int* col;      // streamed index of each entry
  const float* val;    // x of each entry
  const float* ST;     // streamed operand, transposed: replicate r, row l at ST + r*st_rs + l*K4
  long long st_rs;
  float* F;            // fixed operand (R, K, Lf): F + r*f_rs + k*ldf + i
  long long f_rs, ldf;
  int K, K4, Lf, Ls, R;
  int cols_per_wg, n_groups;
  float eps;
  float* num;          // side W: (R, K, Lf)
  int nsteps, loss_entry, loss_exit;
  const float* den_vec;  // (R, K) row sums of S
  float l1, l2, tol;
  int conv_mode;
  double* hstate;      // (R, 2)
  double* part;        // (R, n_groups, 4)
  int* counter;        // (R)
  int* act;            // (R)
  int* iters;          // (R)
  const int* active;   // (R) gate
  double* loss;        // loss-only launches: (R, n_groups)
  double xsum;
};

template <int CTRL>
__device__ __forceinline__ float sk_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// Usage-side tail, called by every thread of the workgroup: workgroup partials (iterate
// change d2 / o2, block objective at entry / exit) -> the replicate's stopping rule (as
// beta_planes.hip bp_kernel: the last workgroup of the replicate to arrive decides).
// `sred`: 4 * (NTH / 64) doubles of LDS, `s_last`: one int of LDS.
template <int NTH>
__device__ __forceinline__ void sk_tail(const SkParams& p, int rep, int grp, float d2, float o2,
                                        double f_entry, double f_exit, double* sred,
                                        int* s_last) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  {
    const double v0 = wave_sum((double)d2), v1 = wave_sum((double)o2);
    const double v2 = wave_sum(f_entry), v3 = wave_sum(f_exit);
    if (lane == 0) {
      sred[wave * 4 + 0] = v0;
      sred[wave * 4 + 1] = v1;
      sred[wave * 4 + 2] = v2;
      sred[wave * 4 + 3] = v3;
    }
    __syncthreads();
  }
  constexpr int kW = NTH / 64;
  if (p.loss && tid == 0) {
    double tot = 0.0;
    for (int w = 0; w < kW; ++w) tot += sred[w * 4 + 3];
    p.loss[(long long)rep * p.n_groups + grp] = tot;
  }
  if (!p.part) return;
  if (tid == 0) {
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int w = 0; w < kW; ++w)
      for (int v = 0; v < 4; ++v) acc[v] += sred[w * 4 + v];
    double* pp = p.part + ((long long)rep * p.n_groups + grp) * 4;
    for (int v = 0; v < 4; ++v) pp[v] = acc[v];
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const int prev = __hip_atomic_fetch_add(p.counter + rep, 1, __ATOMIC_RELAXED,
                                            __HIP_MEMORY_SCOPE_AGENT);
    *s_last = (prev == p.n_groups - 1);
  }
  __syncthreads();
  if (*s_last && tid == 0) {
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    double tot[4] = {0.0, 0.0, 0.0, 0.0};
    const double* pr = p.part + (long long)rep * p.n_groups * 4;
    for (int g2 = 0; g2 < p.n_groups; ++g2)
      for (int v = 0; v < 4; ++v)
        tot[v] += __hip_atomic_load(pr + 4 * g2 + v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    tot[2] -= p.xsum;
    tot[3] -= p.xsum;
    if (p.conv_mode == 1) {
      double* hs = p.hstate + 2 * (long long)rep;
      const double f_prev = p.loss_entry ? tot[2] : hs[0];
      if ((p.loss_entry || hs[1] > 0.0) && fabs(f_prev - tot[3]) <= (double)p.tol * fabs(f_prev))
        p.act[rep] = 0;
      hs[0] = tot[3];
      hs[1] = hs[1] + 1.0;
    } else if (p.nsteps > 0) {
      const double rel = sqrt(tot[0]) / (sqrt(tot[1]) + (double)p.eps);
      if (rel < (double)p.tol) p.act[rep] = 0;
    }
    if (p.iters) p.iters[rep] += p.nsteps;
    p.counter[rep] = 0;
  }
}

// sparse_kl_wide.hip: 33 <= K <= 64, same parameters and launch geometry as sk_kernel
hipError_t sk_wide_run(int side, const SkParams& p, hipStream_t s);
// sparse_kl_xwide.hip: 65 <= K <= 128, likewise
hipError_t sk_xwide_run(int side, const SkParams& p, hipStream_t s);

}  // namespace cnmf
