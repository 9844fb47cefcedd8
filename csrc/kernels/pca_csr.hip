// Sparse PCA over the device CSR (reference preprocess.py:310 runs scanpy's dense PCA on
// the host): the covariance C = T(A)^T T(A) - n mu mu^T and the scores T(A) V - mu V are
// sums over the stored entries, so neither needs the dense (cells x genes) matrix.
//
//  * csr_gram      G = T(A)^T T(A) (nh x nh, float64) as sparse outer products.  The
//                  kept, transformed entries arrive packed by 64-wide output-column tile
//                  (ops/sparse.py: csr_transform + a stable sort by tile): for tile t a
//                  CSR of (local column, value) over the n rows, row pointers
//                  tptr[t * n + row] .. tptr[t * n + row + 1].  One workgroup of 4 waves
//                  per (tile pair I <= J, row slab); each wave owns a private 64 x 64
//                  float64 accumulator in LDS and takes the 64-row chunks w, w+4, ... of
//                  the slab in order, rows in order within a chunk.  For a row with na entries in tile I and nb in tile J the
//                  lanes enumerate the na * nb pairs 64 at a time and add a_i * b_j into
//                  acc[i][j]: the columns of a row are distinct, so the lanes of one
//                  instruction never share an address, and an address only ever sees
//                  its own wave.  The diagonal pair computes the full square.  The four
//                  replicas are summed in wave order into part[slab], at (I, J) and
//                  transposed at (J, I); the slabs are summed in fixed order by the
//                  caller.  No atomics: the same bits on every run, and G == G^T bitwise
//                  (a_i * b_j == b_j * a_i, added in the same row order on both sides).
//  * csr_project   out[r, :] = sum_j v'_j V[c'_j, :] - shift[:] (float64): one wave per
//                  row, lane = component (<= 64 per launch), the row's entries in stored
//                  order, each row of V one coalesced read.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"

namespace cnmf {

constexpr int kGrTile = 64;       // output columns per tile
constexpr int kGrLd = 65;         // accumulator row stride in doubles: acc[i][j] with equal j
                                  // and different i would all hit one bank at stride 64
constexpr int kGrWaves = 4;
constexpr int kGrAcc = kGrTile * kGrLd;   // doubles per wave: 4 x 33,280 B = 130 KiB of LDS
constexpr int kGrMinRows = 256;   // rows per slab at least, a 64-row chunk per wave (small n: fewer slabs)
constexpr int kGrTarget = 512;    // workgroups aimed at: two per CU

// A row's entries in tiles I and J, one per lane (local column -1 beyond the segment).
struct GramRow {
  int na, nb, ca, cb;
  double va, vb;
};

__device__ __forceinline__ int seg_len(long long d) {
  return d < 0 ? 0 : (d > kGrTile ? kGrTile : (int)d);
}

// Row k of the chunk whose pointers the lanes hold (k is wave-uniform; every lane calls).
__device__ __forceinline__ GramRow gram_row(const int* __restrict__ lcol,
                                            const double* __restrict__ val, long long a0,
                                            long long b0, int na, int nb, int k, bool diag,
                                            int lane) {
  GramRow r;
  const long long ka0 = __shfl(a0, k, kWave);
  r.na = __shfl(na, k, kWave);
  r.ca = -1;
  r.va = 0.0;
  if (lane < r.na) {
    r.ca = lcol[ka0 + lane];
    r.va = val[ka0 + lane];
  }
  if (diag) {
    r.nb = r.na;
    r.cb = r.ca;
    r.vb = r.va;
    return r;
  }
  const long long kb0 = __shfl(b0, k, kWave);
  r.nb = __shfl(nb, k, kWave);
  r.cb = -1;
  r.vb = 0.0;
  if (lane < r.nb) {
    r.cb = lcol[kb0 + lane];
    r.vb = val[kb0 + lane];
  }
  return r;
}

__global__ void __launch_bounds__(256) csr_gram_kernel(const long long* __restrict__ tptr,
                                                       const int* __restrict__ lcol,
                                                       const double* __restrict__ val, int n,
                                                       int nh, int ntile, int rows_per_slab,
                                                       double* __restrict__ part) {
  extern __shared__ __attribute__((aligned(16))) double gacc[];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  double* acc = gacc + (size_t)wave * kGrAcc;
  // blockIdx.x -> tile pair (I, J), I <= J, rows of the upper triangle in order
  int I = 0, p = blockIdx.x;
  while (I < ntile && p >= ntile - I) {
    p -= ntile - I;
    ++I;
  }
  const int J = I + p;
  if (I >= ntile || J >= ntile) return;   // uniform over the workgroup, before any barrier
  const bool diag = I == J;
  const int slab = blockIdx.y;
  const long long r0 = (long long)slab * rows_per_slab;
  const long long r1 = r0 + rows_per_slab < n ? r0 + rows_per_slab : n;
  for (int e = threadIdx.x; e < kGrWaves * kGrAcc; e += 256) gacc[e] = 0.0;
  __syncthreads();
  const long long* pI = tptr + (long long)I * n;
  const long long* pJ = tptr + (long long)J * n;
  // A wave takes the 64-row chunks w, w+4, ... of the slab in order.  Lane l loads the row
  // pointers of the chunk's row l (coalesced: one latency per 64 rows, not four per row);
  // the rows with entries in both tiles are then walked in order, the entries of the next
  // such row requested before the pairs of the current one are accumulated.
  for (long long c0 = r0 + (long long)wave * kWave; c0 < r1; c0 += kGrWaves * kWave) {
    const long long myrow = c0 + lane;
    long long a0 = 0, b0 = 0;
    int na = 0, nb = 0;
    if (myrow < r1) {
      a0 = pI[myrow];
      // distinct columns per row: a tile holds at most 64 entries of a row
      na = seg_len(pI[myrow + 1] - a0);
      if (!diag) {
        b0 = pJ[myrow];
        nb = seg_len(pJ[myrow + 1] - b0);
      } else {
        nb = na;
      }
    }
    unsigned long long live = __ballot(na > 0 && nb > 0);   // wave-uniform
    GramRow cur = {}, nxt = {};
    bool have = live != 0;
    if (have) {
      const int k = __ffsll((long long)live) - 1;
      live &= live - 1;
      cur = gram_row(lcol, val, a0, b0, na, nb, k, diag, lane);
    }
    while (have) {
      const bool more = live != 0;
      if (more) {
        const int k = __ffsll((long long)live) - 1;
        live &= live - 1;
        nxt = gram_row(lcol, val, a0, b0, na, nb, k, diag, lane);
      }
      const int np = cur.na * cur.nb;     // <= 4096
      const float rnb = 1.0f / (float)cur.nb;
      for (int p0 = 0; p0 < np; p0 += 64) {
        const int q = p0 + lane;
        const bool ok = q < np;
        const int qq = ok ? q : 0;
        // qq / nb: (qq + 0.5) / nb is at least 2^-7 away from an integer and below 2^12,
        // the float product is within 2^-11 of it
        const int i = (int)(((float)qq + 0.5f) * rnb) & 63;
        const int j = (qq - i * cur.nb) & 63;
        // every lane takes part in the shuffles; only valid pairs touch LDS
        const int ci = __shfl(cur.ca, i, kWave), cj = __shfl(cur.cb, j, kWave);
        const double x = __shfl(cur.va, i, kWave), y = __shfl(cur.vb, j, kWave);
        if (ok && (unsigned)ci < (unsigned)kGrTile && (unsigned)cj < (unsigned)kGrTile)
          acc[ci * kGrLd + cj] += x * y;
      }
      cur = nxt;
      have = more;
    }
  }
  __syncthreads();
  double* out = part + (size_t)slab * nh * nh;
  for (int e = threadIdx.x; e < kGrTile * kGrTile; e += 256) {
    const int i = e >> 6, j = e & 63;
    const int gi = I * kGrTile + i, gj = J * kGrTile + j;
    if (gi >= nh || gj >= nh) continue;
    const int a = i * kGrLd + j;
    const double s = ((gacc[a] + gacc[kGrAcc + a]) + gacc[2 * kGrAcc + a]) + gacc[3 * kGrAcc + a];
    out[(size_t)gi * nh + gj] = s;
    if (!diag) out[(size_t)gj * nh + gi] = s;
  }
}

template <class TV>
__global__ void __launch_bounds__(256) csr_project_kernel(
    const long long* __restrict__ indptr, const int* __restrict__ indices,
    const TV* __restrict__ vals, int n, int nh, const int* __restrict__ col_map,
    const double* __restrict__ V, int ncomp, const double* __restrict__ shift,
    double* __restrict__ out) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (row >= n) return;   // whole waves leave; the kernel has no barrier
  const bool comp = lane < ncomp;
  double acc = 0.0;
  const long long e = indptr[row + 1];
  for (long long j0 = indptr[row]; j0 < e; j0 += 64) {
    // 64 entries per trip, one per lane, then walked in stored order by all lanes
    const long long j = j0 + lane;
    int c = -1;
    double v = 0.0;
    if (j < e) {
      c = indices[j];
      if (col_map) c = col_map[c];
      if ((unsigned)c >= (unsigned)nh) c = -1;   // dropped (or outside V): skipped below
      v = (double)vals[j];
    }
    const int cnt = e - j0 < 64 ? (int)(e - j0) : 64;
    for (int k = 0; k < cnt; ++k) {
      const int ck = __shfl(c, k, kWave);
      const double vk = __shfl(v, k, kWave);
      if (ck >= 0 && comp) acc = fma(vk, V[(size_t)ck * ncomp + lane], acc);
    }
  }
  if (comp) out[(size_t)row * ncomp + lane] = shift ? acc - shift[lane] : acc;
}

}  // namespace cnmf

extern "C" int cnmf_csr_gram_min_rows() { return cnmf::kGrMinRows; }

// Slabs of rows per tile pair, from the shape alone (the reduction order never depends on
// the device): enough workgroups to cover the chip about twice, at least kGrMinRows rows
// each.  The partials stay small by construction: S <= kGrTarget / P + 1 with P about
// (nh / 64)^2 / 2 tile pairs, so S nh^2 8 bytes is at most kGrTarget 2 64^2 8 = 32 MiB plus
// one nh x nh matrix.
extern "C" int cnmf_csr_gram_slabs(int n, int nh) {
  if (n <= 0 || nh <= 0) return 1;
  const long long T = ((long long)nh + cnmf::kGrTile - 1) / cnmf::kGrTile;
  const long long P = T * (T + 1) / 2;
  long long S = (cnmf::kGrTarget + P - 1) / P;
  const long long by_rows = ((long long)n + cnmf::kGrMinRows - 1) / cnmf::kGrMinRows;
  if (S > by_rows) S = by_rows;
  return S < 1 ? 1 : (int)S;
}

extern "C" hipError_t cnmf_csr_gram(const long long* tptr, const int* lcol, const double* val,
                                    int n, int nh, double* part, hipStream_t stream) {
  if (n <= 0 || nh <= 0) return hipSuccess;
  const long long T = ((long long)nh + cnmf::kGrTile - 1) / cnmf::kGrTile;
  const long long P = T * (T + 1) / 2;
  if (P > 0x7fffffffLL) return hipErrorInvalidValue;
  const int S = cnmf_csr_gram_slabs(n, nh);
  const int rps = (n + S - 1) / S;
  const size_t lds = (size_t)cnmf::kGrWaves * cnmf::kGrAcc * sizeof(double);
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cnmf::csr_gram_kernel),
                                     hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cnmf::csr_gram_kernel, dim3((unsigned)P, (unsigned)S), dim3(256), lds,
                     stream, tptr, lcol, val, n, nh, (int)T, rps, part);
  return hipGetLastError();
}

extern "C" hipError_t cnmf_csr_project(const long long* indptr, const int* indices,
                                       const void* vals, int vals_f64, int n, int nh,
                                       const int* col_map, const double* V, int ncomp,
                                       const double* shift, double* out, hipStream_t stream) {
  if (n <= 0) return hipSuccess;
  if (ncomp < 1 || ncomp > 64 || nh < 1) return hipErrorInvalidValue;
  const dim3 grid((n + 3) / 4);
  if (vals_f64)
    hipLaunchKernelGGL(cnmf::csr_project_kernel<double>, grid, dim3(256), 0, stream, indptr,
                       indices, (const double*)vals, n, nh, col_map, V, ncomp, shift, out);
  else
    hipLaunchKernelGGL(cnmf::csr_project_kernel<float>, grid, dim3(256), 0, stream, indptr,
                       indices, (const float*)vals, n, nh, col_map, V, ncomp, shift, out);
  return hipGetLastError();
}
