// Sparse KL MU over a CSR matrix for 65 <= K <= 128 (gfx950 / CDNA4): sparse_kl_wide.hip's
// kernel with the components of a column split over more lanes of its 16-lane DPP row.  A
// row is 16 / KS entry slots x KS component slices: lane KS s + h handles entry slot s and
// the components [h KH, h KH + KH), KH = 4 NQH, so a lane holds at most 16 usages,
// accumulators and gathered floats per entry -- the registers of sparse_kl_wide.hip.  The
// partial dot products of an entry are added across its KS lanes (quad_perm, quad_perm,
// row_half_mirror DPP adds; + row_mirror at KS = 16) before q = x / p; at KS = 8 the K sums
// are then added over the two slots of a slice with one row_ror:8.  Every step adds two
// operands that both lanes of the exchange hold, so all lanes that keep a copy of a usage
// get bit-identical sums and the copies stay equal.  A row walks 8 entries per batch.  Same
// SkParams, launch geometry (XCD map, columns per workgroup, LDS staging rule), `active`
// gate and stopping-rule tail as sparse_kl.hip.  At K = 128 the LDS variant holds 256
// streamed rows: the spectra side of 100 replicates x 2,000 genes is 16 groups of 128 genes
// per replicate, 1,600 workgroups over 256 CUs.
//
// Registers (hipcc -Rpass-analysis=kernel-resource-usage, no scratch, no AGPRs anywhere):
//   K4 68..96   (KS 8, NQH 3): usage 183 (LDS, 512 threads) / 187 VGPRs, spectra 160 / 170
//   K4 100..128 (KS 8, NQH 4): usage 225 (LDS, 512 threads) / 241 VGPRs, spectra 207 / 212
// KS = 16 (one entry slot, NQH 2, 8 entries per lane per batch) fits as well -- usage 202 /
// 223, spectra 125 / 135 -- but leaves 6 of 16 lanes idle at K4 = 80 and pays a four-step
// entry sum per entry: measured on 100 replicates x 5,000 cells x 2,000 genes at 8 %
// density, a 10-step usage block takes 25.1 ms against 20.5 (K = 80) and 38.7 against 37.0
// (K = 128), the spectra numerators 2.89 against 2.17 and 4.21 against 3.61 ms.
#include <hip/hip_runtime.h>

#include "common.h"
#include "sparse_kl.h"

namespace cnmf {

// sum over the KS lanes of a DPP row that hold the slices of one entry slot
template <int KS>
__device__ __forceinline__ float sk_xentry_sum(float v) {
  v += sk_dpp<0xB1>(v);                  // quad_perm [1,0,3,2]
  v += sk_dpp<0x4E>(v);                  // quad_perm [2,3,0,1]
  v += sk_dpp<0x141>(v);                 // row_half_mirror
  if (KS == 16) v += sk_dpp<0x140>(v);   // row_mirror
  return v;
}

// sum over the 16 / KS lanes of a DPP row that share a component slice; every one of them
// receives the same bits
template <int KS>
__device__ __forceinline__ float sk_xslice_sum(float v) {
  if (KS == 8) v += sk_dpp<0x128>(v);    // row_ror:8
  return v;
}

// NQH: float4 quads per slice, kSkU: entries per lane per batch (independent chains for
// latency).  Quads that lie past the row (K4 < 4 KS NQH: the last slices, whole slices at
// the low ranks of a bucket) re-read the row's last quad (a valid address) against zero
// usages: they add nothing to p, and their sums are never stored.
template <int KS, int NQH, int kSkU, bool UPD, bool LDS>
__global__ void __launch_bounds__(LDS ? kSkThreadsL : kSkThreads) sk_xwide_kernel(SkParams p) {
  constexpr int KH = 4 * NQH;
  constexpr int kSkSlots = kSkRow / KS;   // entry slots per DPP row
  constexpr int NTH = LDS ? kSkThreadsL : kSkThreads;
  constexpr int NCOL = NTH / kSkRow;
  __shared__ double sred[4 * (NTH / 64)];
  __shared__ int s_last;
  extern __shared__ __attribute__((aligned(16))) float sk_lds[];
  // XCD-aware map of sparse_kl.hip: replicate r runs on XCD r % 8, its replicates interleaved
  const int b = blockIdx.x, xcd = b & 7, local = b >> 3;
  const int RX = (p.R + 7) >> 3;
  const int rep = (local % RX) * 8 + xcd;
  const int grp = local / RX;
  if (rep >= p.R || grp >= p.n_groups) return;
  if (p.active && p.active[rep] == 0) return;
  const int tid = threadIdx.x;
  const int rl = tid & (kSkRow - 1), rc = tid / kSkRow;
  const int sl = rl & (KS - 1), slot = rl / KS;
  const int K = p.K, K4 = p.K4;
  const int k0 = sl * KH;                                     // first component of the slice
  int voff[NQH];                                              // quad offsets in a row
#pragma unroll
  for (int v = 0; v < NQH; ++v) voff[v] = min(k0 + 4 * v, K4 - 4);
  const float* __restrict__ ST = p.ST + (long long)rep * p.st_rs;
  if (LDS) {
    const float4* src = reinterpret_cast<const float4*>(ST);
    float4* dst = reinterpret_cast<float4*>(sk_lds);
    const int n4 = p.Ls * (K4 >> 2);
    for (int i = tid; i < n4; i += NTH) dst[i] = src[i];
    __syncthreads();
    ST = sk_lds;
  }
  float* __restrict__ F = p.F + (long long)rep * p.f_rs;
  const float* dv = p.den_vec ? p.den_vec + (long long)rep * K : nullptr;
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
    for (int k = 0; k < KH; ++k) h[k] = k0 + k < K ? F[(long long)(k0 + k) * p.ldf + c] : 0.f;
    sk_f2 h2[KH / 2];
    const int beg = p.rowptr[c], end = p.rowptr[c + 1];
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
      // as sparse_kl.hip: the index / value loads of batch t + 1 are in flight while batch
      // t computes, and the row gathers of a batch are issued together
      int jn[kSkU];
      float xn[kSkU];
      auto load_jx = [&](int t) {
#pragma unroll
        for (int u = 0; u < kSkU; ++u) {
          // unconditional loads, clamped into the column (trips > 0 means end > beg)
          const int e = beg + (t * kSkU + u) * kSkSlots + slot;
          const int ec = min(e, end - 1);
          jn[u] = p.col[ec];
          xn[u] = p.val[ec];     // masked where used
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
          const float ps = sk_xentry_sum<KS>(p2.x + p2.y);   // + the other slices' partials
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
        // the KS lanes of an entry hold the same ls: slice 0 counts it; the objective's linear
        // part sum_k h_k (sum_l S_kl) once per column, each slice its own components
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
          acc[2 * k] = sk_xslice_sum<KS>(acc2[k].x);
          acc[2 * k + 1] = sk_xslice_sum<KS>(acc2[k].y);
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
          float* o = p.num + (long long)rep * K * p.Lf + c;
#pragma unroll
          for (int k = 0; k < KH; ++k)
            if (k0 + k < K && slot == (k & (kSkSlots - 1))) o[(long long)(k0 + k) * p.Lf] = acc[k];
        }
      }
    }
    if (UPD && p.nsteps > 0) {
#pragma unroll
      for (int k = 0; k < KH; ++k)
        if (k0 + k < K && slot == (k & (kSkSlots - 1))) F[(long long)(k0 + k) * p.ldf + c] = h[k];
    }
  }
  if (!UPD) return;
  sk_tail<NTH>(p, rep, grp, d2, o2, f_entry, f_exit, sred, &s_last);
}

template <int KS, int NQH, int U, bool UPD, bool LDS>
hipError_t sk_xwide_launch(const SkParams& p, hipStream_t s) {
  const int RX = (p.R + 7) / 8;
  const dim3 grid((unsigned)(8 * RX * p.n_groups));
  const size_t lds = LDS ? (size_t)p.Ls * 4 * p.K4 : 0;
  if (LDS) {
    static bool attr_done = false;
    if (!attr_done) {
      const hipError_t e = hipFuncSetAttribute(
          reinterpret_cast<const void*>(&sk_xwide_kernel<KS, NQH, U, UPD, LDS>),
          hipFuncAttributeMaxDynamicSharedMemorySize, kSkLdsBytes);
      if (e != hipSuccess) return e;
      attr_done = true;
    }
  }
  hipLaunchKernelGGL((sk_xwide_kernel<KS, NQH, U, UPD, LDS>), grid,
                     dim3(LDS ? kSkThreadsL : kSkThreads), lds, s, p);
  return hipGetLastError();
}

template <bool UPD, bool LDS>
hipError_t sk_xwide_launch_k(const SkParams& p, hipStream_t s) {
  switch ((p.K4 + 15) / 16) {
    case 5:                                                      // K4 68 .. 80
    case 6: return sk_xwide_launch<8, 3, 4, UPD, LDS>(p, s);   // K4 84 .. 96
    case 7:                                                      // K4 100 .. 112
    case 8: return sk_xwide_launch<8, 4, 4, UPD, LDS>(p, s);   // K4 116 .. 128
    default: return hipErrorInvalidValue;
  }
}

hipError_t sk_xwide_run(int side, const SkParams& p, hipStream_t s) {
  if (p.K <= kSkWideMaxK || p.K > kSkXWideMaxK) return hipErrorInvalidValue;
  const bool lds = (long long)p.Ls * p.K4 * 4 <= kSkLdsBytes;
  if (side == 1)
    return lds ? sk_xwide_launch_k<false, true>(p, s) : sk_xwide_launch_k<false, false>(p, s);
  return lds ? sk_xwide_launch_k<true, true>(p, s) : sk_xwide_launch_k<true, false>(p, s);
}

}  // namespace cnmf
