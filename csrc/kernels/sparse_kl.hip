// KL-divergence MU over a CSR matrix (gfx950 / CDNA4), replicate-batched, K <= 128: the
// sparse counterpart of beta_planes.hip for X below ~30 % density (HVG count matrices are
// typically 5-30 % non-zero).  KL is the one beta-divergence whose MU statistics only
// touch the non-zeros of X: with Q = X / P, num = S Q vanishes wherever x = 0, the
// denominator S 1 is a row sum of S, and D_KL(X | P) = sum_nz x log(x / p) - sum x +
// sum_k (sum F_k)(sum S_k).  So work and bytes scale with nnz instead of the dense
// element count (sklearn/decomposition/_nmf.py:526-728 computes the same MU step densely;
// SURVEY.md §2.4 G6, docs/ARCHITECTURE.md "Sparse KL").
//
// Layout: one 16-lane DPP row per fixed-axis column (a cell on the usage side H, a gene on
// the spectra side W), 16 columns per workgroup in flight (32 in the LDS variant).  A row is
// 16 / KS entry slots x KS component slices: lane KS s + h handles entry slot s and the
// components [h KH, h KH + KH), KH = 4 NQH, so a lane holds KH usages, accumulators and
// gathered floats per entry.  The row walks its column's CSR entries 16 / KS x U at a time
// (U = 4 per lane, next batch's indices prefetched); a lane gathers its KH contiguous floats
// of the streamed operand's row S^T[j] (K floats, zero-padded to a multiple of 4, float4
// loads; L2-resident, the replicates of one XCD sharing its L2 through the XCD-aware block
// map, or staged in LDS), forms its part of p = eps + S^T[j] . f exactly in fp32
// (v_pk_fma_f32 pairs: no MFMAs here, so packed VALU is the full-rate path), adds the parts
// of the KS slices (DPP adds), q = x / p, and accumulates q S^T[j]; DPP adds over the slots
// of a slice reduce the K sums.  Every DPP step adds two operands that both lanes of the
// exchange hold, so all lanes that keep a copy of a usage get bit-identical sums and the
// copies stay equal.  Unlike the dense kernel there is no shared panel, so the usage side
// runs all `nsteps` MU steps of a column back to back with the usages in registers.  The
// block-objective stopping rule is the dense kernel's (last workgroup of the replicate to
// arrive decides, cdna_hip_programming.md G16).
//
// Chunk-batched mode of the usage side (cnmf_sk_refit_step, the KL refit of models/refit.py):
// "replicate" r is row chunk r of one matrix -- its CSR rows start rowptr + r * row_rs, its
// usages are the columns [r c, (r + 1) c) of one (K x n) array -- and all chunks gather from
// one S^T / den_vec.  One launch is one MU step of every chunk whose flag is set, then the
// iterate-change rule per chunk; with the operand shared the XCD pinning has no purpose, so
// the blocks interleave over the chunks and two chunks still use every XCD.  A run-time field:
// registers, scratch and occupancy of every instantiation are what they were without it
// (profiles/p8_kl_refit.txt), and with it off a launch is bit for bit the former one.
//
// Buckets, <KS, NQH> by padded rank K4, and their VGPRs (hipcc
// -Rpass-analysis=kernel-resource-usage; usage LDS (512 threads) / L2, spectra LDS / L2; no
// scratch and no AGPRs anywhere but the 256-VGPR usage kernels at K4 = 28 and 32):
//   K4 <= 32    <1, K4/4>: every lane holds all K4 components (~6.5 K4 VGPRs: 256 and
//                          spills at K4 = 32, which cannot grow with two waves per SIMD)
//   K4 36..48   <4, 3>: usage 161 / 165, spectra 81 / 79
//   K4 52..64   <4, 4>: usage 196 / 212, spectra 87 / 91
//   K4 68..96   <8, 3>: usage 161 / 165, spectra 160 / 170
//   K4 100..128 <8, 4>: usage 196 / 212, spectra 207 / 212
// (all 48 kernels: profiles/p7_sparse_kl_unified.txt).  At K = 128 the LDS variant holds 256
// streamed rows: the spectra side of 100 replicates x 2,000 genes is 16 groups of 128 genes
// per replicate, 1,600 workgroups over 256 CUs.
//
// Measured and rejected:
//  * KS = 2 with 4 entries per lane for K4 36..64 does not fit: 256 VGPRs plus 12-256 B of
//    scratch (LDS) or 9-66 AGPRs at one wave per SIMD (L2) from K4 = 44 up.
//  * KS = 16 (one entry slot, NQH 2, 8 entries per lane per batch) for K4 68..128 fits --
//    usage 202 / 223, spectra 125 / 135 VGPRs -- but leaves 6 of 16 lanes idle at K4 = 80
//    and pays a four-step entry sum per entry: on 100 replicates x 5,000 cells x 2,000 genes
//    at 8 % density, a 10-step usage block takes 25.1 ms against 20.5 (K = 80) and 38.7
//    against 37.0 (K = 128), the spectra numerators 2.89 against 2.17 and 4.21 against
//    3.61 ms.
//  * Taking an XCD's replicates one after the other instead of interleaved (13 x 384-512 KB
//    of S^T at R = 100 exceed one 4 MB L2): +3..11 % at K = 48, -1..3 % at K = 64
//    (profiles/p2_kl_wide_block_order.txt).
#include <hip/hip_runtime.h>

#include "common.h"

namespace cnmf {

typedef float sk_f2 __attribute__((ext_vector_type(2)));

constexpr int kSkThreads = 256;                 // global-gather variant
constexpr int kSkThreadsL = 512;                // LDS variant (one workgroup per CU)
constexpr int kSkRow = 16;                      // lanes per fixed column (one DPP row)
constexpr int kSkCols = kSkThreads / kSkRow;    // columns in flight per workgroup
constexpr int kSkLdsBytes = 128 * 1024;         // LDS budget for the staged S^T rows
constexpr int kSkMaxK = 128;

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
  // chunk-batched usage step (a refit: many row chunks against one shared fixed S): replicate
  // r is chunk r, reads the CSR rows from rowptr + r * row_rs on and gathers from the one
  // S^T / den_vec (no replicate stride); 0 / 0 everywhere else
  int chunk, row_rs;
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

// whether a launch stages the Ls rows of S^T in LDS (gathers from LDS instead of L2: 48 B
// per non-zero at K = 10 made the L2-gather variant bandwidth-bound)
inline bool sk_use_lds(int Ls, int K4) { return (long long)Ls * K4 * 4 <= kSkLdsBytes; }

template <int CTRL>
__device__ __forceinline__ float sk_dpp(float v) {
  return __builtin_bit_cast(
      float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xF, 0xF, true));
}

// sum over the KS lanes of a DPP row that hold the slices of one entry slot
template <int KS>
__device__ __forceinline__ float sk_entry_sum(float v) {
  if (KS >= 2) v += sk_dpp<0xB1>(v);    // quad_perm [1,0,3,2]
  if (KS >= 4) v += sk_dpp<0x4E>(v);    // quad_perm [2,3,0,1]
  if (KS >= 8) v += sk_dpp<0x141>(v);   // row_half_mirror
  return v;
}

// sum over the 16 / KS lanes of a DPP row that share a component slice; every one of them
// receives the same bits
template <int KS>
__device__ __forceinline__ float sk_slice_sum(float v) {
  if (KS == 1) {
    v += sk_dpp<0xB1>(v);    // quad_perm [1,0,3,2]
    v += sk_dpp<0x4E>(v);    // quad_perm [2,3,0,1]
    v += sk_dpp<0x141>(v);   // row_half_mirror
    v += sk_dpp<0x140>(v);   // row_mirror
  } else {
    v += sk_dpp<0x128>(v);                // row_ror:8
    if (KS == 4) v += sk_dpp<0x124>(v);   // row_ror:4
  }
  return v;
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

// KS: component slices per DPP row, NQH: float4 quads per slice, kSkU: entries per lane per
// batch (independent chains for latency).  Quads that lie past the row (K4 < 4 KS NQH: the
// last slices, whole slices at the low ranks of a bucket) re-read the row's last quad (a
// valid address) against zero usages: they add nothing to p, and their sums are never stored.
// LDS: the replicate's S^T rows [0, Ls) are staged in LDS first, 512 threads so that one
// workgroup per CU still keeps two waves per SIMD.
template <int KS, int NQH, int kSkU, bool UPD, bool LDS>
__global__ void __launch_bounds__(LDS ? kSkThreadsL : kSkThreads) sk_kernel(SkParams p) {
  static_assert(KS == 1 || KS == 4 || KS == 8, "KS 2 and 16 were measured and rejected");
  constexpr int KH = 4 * NQH;
  constexpr int kSkSlots = kSkRow / KS;   // entry slots per DPP row
  constexpr int NTH = LDS ? kSkThreadsL : kSkThreads;
  constexpr int NCOL = NTH / kSkRow;
  __shared__ double sred[4 * (NTH / 64)];
  __shared__ int s_last;
  extern __shared__ __attribute__((aligned(16))) float sk_lds[];
  // XCD-aware map: replicate r runs on XCD r % 8 (all of its workgroups), its replicates
  // interleaved, so its S^T rows are gathered from one L2
  // (chunk mode: the operand is shared, so the chunks interleave and R < 8 of them still
  // spread over every XCD)
  const int b = blockIdx.x, xcd = b & 7, local = b >> 3;
  const int RX = (p.R + 7) >> 3;
  const int rep = p.chunk ? b % p.R : (local % RX) * 8 + xcd;
  const int grp = p.chunk ? b / p.R : local / RX;
  if (rep >= p.R || grp >= p.n_groups) return;
  if (p.active && p.active[rep] == 0) return;
  const int tid = threadIdx.x;
  const int rl = tid & (kSkRow - 1), rc = tid / kSkRow;
  const int sl = rl & (KS - 1), slot = rl / KS;
  const int K = p.K, K4 = KS == 1 ? KH : p.K4;    // one slice: the bucket is the padded rank
  const int k0 = sl * KH;                                     // first component of the slice
  // The slice's first row of F / num goes into the base pointers (kb = k0) and the rows are
  // indexed by the compile-time k, except on the spectra side at KS 8: there the rows are
  // indexed by the run-time k0 + k (ki = k0), which keeps up to 16 row offsets live per lane
  // (160-212 against 81-90 VGPRs) and is 9-10 % faster -- the LDS variant is one 512-thread
  // workgroup per CU whatever its registers (profiles/p7_sparse_kl_unified.txt)
  constexpr bool kRowIdx = KS == 8 && !UPD;
  const int kb = kRowIdx ? 0 : k0, ki = k0 - kb;
  int voff[NQH];                                              // quad offsets in a row
#pragma unroll
  for (int v = 0; v < NQH; ++v) voff[v] = min(k0 + 4 * v, K4 - 4);
  const float* __restrict__ ST = p.ST + (p.chunk ? 0LL : (long long)rep * p.st_rs);
  const int* __restrict__ rowptr = p.rowptr + (long long)rep * p.row_rs;
  if (LDS) {
    const float4* src = reinterpret_cast<const float4*>(ST);
    float4* dst = reinterpret_cast<float4*>(sk_lds);
    const int n4 = p.Ls * (K4 >> 2);
    for (int i = tid; i < n4; i += NTH) dst[i] = src[i];
    __syncthreads();
    ST = sk_lds;
  }
  float* __restrict__ F = p.F + (long long)rep * p.f_rs + (long long)kb * p.ldf;
  const float* dv = p.den_vec ? p.den_vec + (p.chunk ? 0LL : (long long)rep * K) : nullptr;
  float den[KH];
#pragma unroll
  for (int k = 0; k < KH; ++k) den[k] = (dv && k0 + k < K) ? dv[k0 + k] : 0.f;
  const float eps0 = sl == 0 ? p.eps : 0.f;   // eps enters p once, through slice 0

  const bool exit_in_last = p.nsteps >= 2;
  const int n_it = UPD ? p.nsteps + ((p.loss_exit && !exit_in_last) || p.nsteps == 0 ? 1 : 0)
                       : 1;
  double f_entry = 0.0, f_exit = 0.0;
  float d2 = 0.f, o2 = 0.f;
  const int c0 = grp * p.cols_per_wg;
  const int c1 = min(p.Lf, c0 + p.cols_per_wg);
  for (int c = c0 + rc; c < c1; c += NCOL) {
    float h[KH];
#pragma unroll
    for (int k = 0; k < KH; ++k) h[k] = k0 + k < K ? F[(long long)(ki + k) * p.ldf + c] : 0.f;
    sk_f2 h2[KH / 2];
    const int beg = rowptr[c], end = rowptr[c + 1];
    const int trips = (end - beg + kSkSlots * kSkU - 1) / (kSkSlots * kSkU);
    for (int it = 0; it < n_it; ++it) {
      const bool want_num = !UPD || it < p.nsteps;
      const bool is_exit = it == (exit_in_last ? p.nsteps - 1 : p.nsteps);
      const bool is_entry = it == 0 && p.loss_entry && p.nsteps > 0;
      const bool want_loss = UPD && (is_entry || (is_exit && (p.loss_exit || p.nsteps == 0)));
#pragma unroll
      for (int k = 0; k < KH / 2; ++k) h2[k] = sk_f2{h[2 * k], h[2 * k + 1]};
      sk_f2 acc2[KH / 2];
#pragma unroll
      for (int k = 0; k < KH / 2; ++k) acc2[k] = sk_f2{0.f, 0.f};
      float acc[KH];
      float ls = 0.f;
      // batches of kSkU entries per lane: the index / value loads of batch t + 1 are in
      // flight while batch t computes, and the kSkU * NQH row gathers of a batch are
      // issued together (one L2 round trip per batch, not per entry)
      int jn[kSkU];
      float xn[kSkU];
      auto load_jx = [&](int t) {
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
          // unconditional loads (clamped into the column: trips > 0 means end > beg), so
          // the compiler counts them and batch t waits only for its own row gathers
          const int e = beg + (t * kSkU + u) * kSkSlots + slot;
          const int ec = min(e, end - 1);
          jn[u] = p.col[ec];
          xn[u] = p.val[ec];     // masked where used (a select here would wait for it)
        }
      };
      if (trips > 0) load_jx(0);
      for (int t = 0; t < trips; ++t) {
        float x[kSkU];
        sk_f2 s[kSkU][KH / 2];
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
          x[u] = beg + (t * kSkU + u) * kSkSlots + slot < end ? xn[u] : 0.f;
          const float* sj = ST + (long long)jn[u] * K4;
#pragma unroll
          for (int v = 0; v < NQH; ++v) {
            const float4 w = *reinterpret_cast<const float4*>(sj + voff[v]);
            s[u][2 * v] = sk_f2{w.x, w.y};
            s[u][2 * v + 1] = sk_f2{w.z, w.w};
          }
        }
        load_jx(min(t + 1, trips - 1));   // unconditional: the waits below stay exact
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
          sk_f2 p2 = sk_f2{eps0, 0.f};
#pragma unroll
          for (int k = 0; k < KH / 2; ++k) p2 = __builtin_elementwise_fma(s[u][k], h2[k], p2);
          const float ps = sk_entry_sum<KS>(p2.x + p2.y);   // + the other slices' partials
          const float q = x[u] * __builtin_amdgcn_rcpf(ps);
          if (want_loss && x[u] > 0.f) ls += x[u] * __builtin_amdgcn_logf(q);
          if (want_num) {
            const sk_f2 q2 = sk_f2{q, q};
#pragma unroll
            for (int k = 0; k < KH / 2; ++k) acc2[k] = __builtin_elementwise_fma(q2, s[u][k], acc2[k]);
          }
        }
      }
      if (want_loss) {
        // x ln(x/p) summed over the row's entries: the KS lanes of an entry hold the same ls,
        // slice 0 counts it; plus the objective's linear part sum_k h_k (sum_l S_kl) once per
        // column, each slice its own components (-sum x is subtracted per replicate)
        double l = sl == 0 ? 0.69314718055994530942 * (double)ls : 0.0;
        if (slot == 0) {
          float hp = 0.f;
#pragma unroll
          for (int k = 0; k < KH; ++k) hp = fmaf(h[k], den[k], hp);
          l += (double)hp;
        }
        if (is_entry) f_entry += l;
        if (is_exit) f_exit += l;
      }
      if (want_num) {
#pragma unroll
        for (int k = 0; k < KH / 2; ++k) {
          acc[2 * k] = sk_slice_sum<KS>(acc2[k].x);
          acc[2 * k + 1] = sk_slice_sum<KS>(acc2[k].y);
        }
        if (UPD) {
          const bool last = it + 1 == p.nsteps;
#pragma unroll
          for (int k = 0; k < KH; ++k) {
            if (k0 + k < K) {
              float dn = den[k] + p.l1 + p.l2 * h[k];
              if (dn == 0.f) dn = p.eps;
              const float hn = h[k] * (acc[k] / dn);
              if (last && slot == 0) {
                d2 = fmaf(hn - h[k], hn - h[k], d2);
                o2 = fmaf(h[k], h[k], o2);
              }
              h[k] = hn;
            }
          }
        } else {
          // one store per (component, column): the slots of a slice take turns
          float* o = p.num + ((long long)rep * K + kb) * p.Lf + c;
#pragma unroll
          for (int k = 0; k < KH; ++k)
            if (k0 + k < K && slot == (k & (kSkSlots - 1))) o[(long long)(ki + k) * p.Lf] = acc[k];
        }
      }
    }
    if (UPD && p.nsteps > 0) {
#pragma unroll
      for (int k = 0; k < KH; ++k)
        if (k0 + k < K && slot == (k & (kSkSlots - 1))) F[(long long)(ki + k) * p.ldf + c] = h[k];
    }
  }
  if (!UPD) return;
  sk_tail<NTH>(p, rep, grp, d2, o2, f_entry, f_exit, sred, &s_last);
}

template <int KS, int NQH, int U, bool UPD, bool LDS>
hipError_t sk_launch(const SkParams& p, hipStream_t s) {
  const int RX = (p.R + 7) / 8;
  const dim3 grid((unsigned)((p.chunk ? p.R : 8 * RX) * p.n_groups));
  const size_t lds = LDS ? (size_t)p.Ls * 4 * p.K4 : 0;
  if (LDS) {
    static bool attr_done = false;
    if (!attr_done) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&sk_kernel<KS, NQH, U, UPD, LDS>),
          hipFuncAttributeMaxDynamicSharedMemorySize, kSkLdsBytes);
      if (e != hipSuccess) return e;
      attr_done = true;
    }
  }
  hipLaunchKernelGGL((sk_kernel<KS, NQH, U, UPD, LDS>), grid,
                     dim3(LDS ? kSkThreadsL : kSkThreads), lds, s, p);
  return hipGetLastError();
}

// K4 <= 32: one slice of K4 / 4 quads; above it the 16-component buckets of 4 or 8 slices
template <bool UPD, bool LDS>
hipError_t sk_launch_k(const SkParams& p, hipStream_t s) {
  if (p.K4 <= 32) {
    switch (p.K4 / 4) {
      case 1: return sk_launch<1, 1, 4, UPD, LDS>(p, s);
      case 2: return sk_launch<1, 2, 4, UPD, LDS>(p, s);
      case 3: return sk_launch<1, 3, 4, UPD, LDS>(p, s);
      case 4: return sk_launch<1, 4, 4, UPD, LDS>(p, s);
      case 5: return sk_launch<1, 5, 4, UPD, LDS>(p, s);
      case 6: return sk_launch<1, 6, 4, UPD, LDS>(p, s);
      case 7: return sk_launch<1, 7, 4, UPD, LDS>(p, s);
      case 8: return sk_launch<1, 8, 4, UPD, LDS>(p, s);
      default: return hipErrorInvalidValue;
    }
  }
  switch ((p.K4 + 15) / 16) {
    case 3: return sk_launch<4, 3, 4, UPD, LDS>(p, s);   // K4 36 .. 48
    case 4: return sk_launch<4, 4, 4, UPD, LDS>(p, s);   // K4 52 .. 64
    case 5:                                              // K4 68 .. 80
    case 6: return sk_launch<8, 3, 4, UPD, LDS>(p, s);   // K4 84 .. 96
    case 7:                                              // K4 100 .. 112
    case 8: return sk_launch<8, 4, 4, UPD, LDS>(p, s);   // K4 116 .. 128
    default: return hipErrorInvalidValue;
  }
}

template <bool UPD>
hipError_t sk_launch_u(const SkParams& p, hipStream_t s) {
  return sk_use_lds(p.Ls, p.K4) ? sk_launch_k<UPD, true>(p, s) : sk_launch_k<UPD, false>(p, s);
}

}  // namespace cnmf

// padded row length of the transposed streamed operand
extern "C" int cnmf_sk_k4(int K) { return (K + 3) / 4 * 4; }

// whether a launch stages S^T (Ls rows) in LDS
extern "C" int cnmf_sk_lds(int Ls, int K) { return cnmf::sk_use_lds(Ls, cnmf_sk_k4(K)) ? 1 : 0; }

// fixed columns per workgroup: enough workgroups to fill the chip several times over (LDS
// variant: 128, so the staging read is ~1/50 of a usage block's gathers)
extern "C" int cnmf_sk_cols_per_wg(int Lf, int R, int Ls, int K) {
  if (cnmf_sk_lds(Ls, K)) {
    int cols = 128;
    while (cols > cnmf::kSkThreadsL / cnmf::kSkRow && (long long)R * ((Lf + cols - 1) / cols) < 1024)
      cols /= 2;
    return cols;
  }
  int cols = 64;
  while (cols > cnmf::kSkCols && (long long)R * ((Lf + cols - 1) / cols) < 4096) cols /= 2;
  return cols;
}

// side 0 (H: fused nsteps MU steps of F in place + stopping rule; nsteps 0: loss only into
// `loss`), side 1 (W: num = S Q into `num`)
extern "C" hipError_t cnmf_sk_run(
    int side, const int* rowptr, const int* col, const float* val, const float* ST,
    long long st_rs, float* F, long long f_rs, long long ldf, int K, int Lf, int Ls, int R,
    float eps,
    float* num, int nsteps, int loss_entry, int loss_exit, const float* den_vec, float l1,
    float l2, float tol, int conv_mode, double* hstate, double* part, int* counter, int* act,
    int* iters, const int* active, double* loss, double xsum, hipStream_t stream) {
  if (R <= 0 || Lf <= 0) return hipSuccess;
  if (K < 1 || K > cnmf::kSkMaxK || (side != 0 && side != 1) || rowptr == nullptr ||
      ST == nullptr || (reinterpret_cast<uintptr_t>(ST) & 15) != 0 || st_rs % 4 != 0)
    return hipErrorInvalidValue;
  cnmf::SkParams p;
  p.rowptr = rowptr; p.col = col; p.val = val;
  p.ST = ST; p.st_rs = st_rs;
  p.F = F; p.f_rs = f_rs; p.ldf = ldf;
  if (Ls <= 0 || st_rs < (long long)Ls * cnmf_sk_k4(K)) return hipErrorInvalidValue;
  p.K = K; p.K4 = cnmf_sk_k4(K); p.Lf = Lf; p.Ls = Ls; p.R = R;
  p.cols_per_wg = cnmf_sk_cols_per_wg(Lf, R, Ls, K);
  p.n_groups = (Lf + p.cols_per_wg - 1) / p.cols_per_wg;
  p.eps = eps; p.num = num;
  p.nsteps = nsteps; p.loss_entry = loss_entry; p.loss_exit = loss_exit;
  p.den_vec = den_vec; p.l1 = l1; p.l2 = l2; p.tol = tol; p.conv_mode = conv_mode;
  p.hstate = hstate; p.part = part; p.counter = counter; p.act = act; p.iters = iters;
  p.active = active; p.loss = loss; p.xsum = xsum;
  p.chunk = 0; p.row_rs = 0;
  if (side == 1) {
    if (num == nullptr) return hipErrorInvalidValue;
    return cnmf::sk_launch_u<false>(p, stream);
  }
  if (nsteps < 0 || den_vec == nullptr || (part != nullptr && (counter == nullptr || act == nullptr)) ||
      (part != nullptr && conv_mode == 1 && hstate == nullptr) ||
      (nsteps == 0 && loss == nullptr && part == nullptr))
    return hipErrorInvalidValue;
  return cnmf::sk_launch_u<true>(p, stream);
}

// Chunk-batched usage step (a refit with the spectra fixed): one KL MU step of every still
// active chunk of c rows, chunk r = CSR rows [r c, (r + 1) c) of `rowptr` (R c + 1 offsets)
// and the columns [r c, (r + 1) c) of F (K x ldf), all against the one S^T (Ls x K4) /
// den_vec (K); then the iterate-change rule per chunk (conv_mode 0): act[r] cleared, iters[r]
// counted, `part` (R, groups, 4) / `counter` (R) as for cnmf_sk_run.
extern "C" hipError_t cnmf_sk_refit_step(
    const int* rowptr, const int* col, const float* val, const float* ST, float* F,
    long long ldf, int K, int c, int Ls, int R, float eps, const float* den_vec, float l1,
    float l2, float tol, double* part, int* counter, int* act, int* iters,
    hipStream_t stream) {
  if (R <= 0 || c <= 0) return hipSuccess;
  if (K < 1 || K > cnmf::kSkMaxK || Ls <= 0 || rowptr == nullptr || ST == nullptr ||
      (reinterpret_cast<uintptr_t>(ST) & 15) != 0 || F == nullptr || den_vec == nullptr ||
      part == nullptr || counter == nullptr || act == nullptr ||
      ldf < (long long)R * c)
    return hipErrorInvalidValue;
  cnmf::SkParams p;
  p.rowptr = rowptr; p.col = col; p.val = val;
  p.ST = ST; p.st_rs = 0;
  p.F = F; p.f_rs = c; p.ldf = ldf;
  p.K = K; p.K4 = cnmf_sk_k4(K); p.Lf = c; p.Ls = Ls; p.R = R;
  p.cols_per_wg = cnmf_sk_cols_per_wg(c, R, Ls, K);
  p.n_groups = (c + p.cols_per_wg - 1) / p.cols_per_wg;
  if ((long long)R * p.n_groups > 0x7fffffffLL) return hipErrorInvalidValue;
  p.eps = eps; p.num = nullptr;
  p.nsteps = 1; p.loss_entry = 0; p.loss_exit = 0;
  p.den_vec = den_vec; p.l1 = l1; p.l2 = l2; p.tol = tol; p.conv_mode = 0;
  p.hstate = nullptr; p.part = part; p.counter = counter; p.act = act; p.iters = iters;
  p.active = act; p.loss = nullptr; p.xsum = 0.0;
  p.chunk = 1; p.row_rs = c;
  return cnmf::sk_launch_u<true>(p, stream);
}

extern "C" int cnmf_sk_groups(int Lf, int R, int Ls, int K) {
  const int c = cnmf_sk_cols_per_wg(Lf, R, Ls, K);
  return (Lf + c - 1) / c;
}
