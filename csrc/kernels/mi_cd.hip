// Mutual information of a continuous feature against a discrete target, Ross (2014), as
// scikit-learn's ``_compute_mi_cd`` counts it (docs/ARCHITECTURE.md "Mutual information").
//
// The host sorts every feature of a block once (values ascending) and then the permuted
// class codes (stable), so a class is a contiguous segment [seg[c], seg[c+1]) of ``ranks``
// holding the ascending global ranks of its points; the segments are the same for every
// feature.  One thread owns one point q of that class-sorted order:
//   * g = ranks[q] is its position in the sorted values, v = vals[g];
//   * its same-class neighbours are ranks[q -/+ 1..], whose distances ascend on each side:
//     k = min(n_neighbors, N - 1) steps of a two-list merge give r, the k-th smallest;
//   * radius = nextafter(r, 0) and m = #{j : fl((vals[j] - v)^2) <= fl(radius^2)}, the
//     point itself included.  The predicate is monotone on each side of g, so the last
//     index that holds is found by a galloping search outward and a bisection of the final
//     stride; r == 0 (exact duplicates) counts the duplicates and the point.
// psi(m) comes from a table of digamma(1..n); a workgroup sums its 256 values in a fixed
// order (wave shuffles, then the four wave sums in order) into part[f][tile], and a second
// kernel adds a feature's tiles in a fixed order: no float atomics, the same bits every run
// and for every split of the features into blocks.
//
// The sorted row is read through L2 as it lies in memory.  A tile is 256 consecutive points
// of the class order, so their ranks are spread over the whole row: there is no compact
// value window that a tile could stage in LDS, and none is staged.  Every loop has a fixed
// trip bound and every index is clamped into [0, n).
#include <hip/hip_runtime.h>

#include <cstdint>

namespace cnmf {

constexpr int kMiThreads = 256;
constexpr int kMiMaxNeighbors = 8;

__device__ __forceinline__ int mi_clampi(long long i, int n) {
  return i < 0 ? 0 : (i >= n ? n - 1 : (int)i);
}

// last index j in [g, n) (dir = +1) or first in [0, g] (dir = -1) with
// (row[j] - v)^2 <= rad2, given that it holds at g and fails monotonically outward
__device__ __forceinline__ int mi_reach(const double* __restrict__ row, int n, int g, double v,
                                        double rad2, int dir) {
  const int room = dir > 0 ? n - 1 - g : g;     // steps available outward
  int ok = 0;                                   // largest offset known to hold
  int step = 1;
  int bad = room + 1;                           // smallest offset known to fail (or the end)
  for (int it = 0; it < 32; ++it) {             // gallop: offsets 1, 3, 7, ...
    const int t = ok + step;
    if (t > room) break;
    const double d = row[mi_clampi((long long)g + (long long)dir * t, n)] - v;
    if (d * d <= rad2) {
      ok = t;
      step <<= 1;
    } else {
      bad = t;
      break;
    }
  }
  for (int it = 0; it < 32; ++it) {             // bisect (ok, bad)
    if (bad - ok <= 1) break;
    const int t = ok + ((bad - ok) >> 1);
    const double d = row[mi_clampi((long long)g + (long long)dir * t, n)] - v;
    if (d * d <= rad2) ok = t; else bad = t;
  }
  return g + dir * ok;
}

__global__ __launch_bounds__(kMiThreads) void mi_cd_kernel(
    const double* __restrict__ vals, const long long* __restrict__ perm,
    const long long* __restrict__ ranks, const int* __restrict__ cid,
    const int* __restrict__ seg, const double* __restrict__ psi, int n, int nn,
    double* __restrict__ part, int tiles, int* __restrict__ m_out, long long ldm,
    const int* __restrict__ rowmap) {
  __shared__ double wsum[kMiThreads / 64];
  const int f = blockIdx.y;
  const int q = blockIdx.x * kMiThreads + threadIdx.x;
  const double* __restrict__ row = vals + (long long)f * n;
  const long long* __restrict__ rk = ranks + (long long)f * n;
  double term = 0.0;
  if (q < n) {
    const int c = cid[q];
    const int a = max(seg[c], 0), b = min(seg[c + 1], n);
    const int g = mi_clampi(rk[q], n);
    const double v = row[g];
    const int k = min(nn, b - a - 1);
    // merge of the two ascending neighbour-distance lists, k steps
    const double inf = __builtin_huge_val();
    int il = q - 1, ir = q + 1;
    double dl = il >= a ? v - row[mi_clampi(rk[il], n)] : inf;
    double dr = ir < b ? row[mi_clampi(rk[ir], n)] - v : inf;
    double r = 0.0;
    for (int t = 0; t < kMiMaxNeighbors; ++t) {
      if (t >= k) break;
      if (dl <= dr) {
        r = dl;
        --il;
        dl = il >= a ? v - row[mi_clampi(rk[il], n)] : inf;
      } else {
        r = dr;
        ++ir;
        dr = ir < b ? row[mi_clampi(rk[ir], n)] - v : inf;
      }
    }
    // nextafter(r, 0) of a finite r >= 0: one step down in the bit pattern
    double radius = 0.0;
    if (r > 0.0 && r < inf) radius = __longlong_as_double(__double_as_longlong(r) - 1);
    const double rad2 = radius * radius;
    const int hi = mi_reach(row, n, g, v, rad2, 1);
    const int lo = mi_reach(row, n, g, v, rad2, -1);
    const int m = hi - lo + 1;                  // 1..n
    term = psi[mi_clampi(m - 1, n)];
    if (m_out != nullptr) {
      const long long src = perm[(long long)f * n + g];
      m_out[(long long)rowmap[mi_clampi(src, n)] * ldm + f] = m;
    }
  }
  // fixed-order sum of the workgroup's 256 terms
  for (int off = 32; off > 0; off >>= 1) term += __shfl_down(term, off, 64);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    double s = wsum[0];
    for (int w = 1; w < kMiThreads / 64; ++w) s += wsum[w];
    part[(long long)f * tiles + blockIdx.x] = s;
  }
}

// sum[f] = part[f][0] + ... in a fixed order: lane l adds tiles l, l + 64, ... and the 64
// lane sums fold by halves
__global__ __launch_bounds__(64) void mi_cd_sum_kernel(const double* __restrict__ part,
                                                        int tiles, double* __restrict__ sum) {
  const int f = blockIdx.x;
  double s = 0.0;
  for (int t = threadIdx.x; t < tiles; t += 64) s += part[(long long)f * tiles + t];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (threadIdx.x == 0) sum[f] = s;
}

}  // namespace cnmf

extern "C" int cnmf_mi_cd_tile() { return cnmf::kMiThreads; }

// vals (F, n) ascending rows; perm (F, n) the source point of every sorted position; ranks
// (F, n) the sorted positions in class order; cid (n) the class of every class-order slot;
// seg (classes + 1) the class offsets; psi (n) = digamma(1..n); part (F, tiles) scratch with
// tiles = ceil(n / tile); sum (F) receives sum_i psi(m_i).  m_out (optional): m of source
// point p of feature f goes to m_out[rowmap[p] * ldm + f].
extern "C" hipError_t cnmf_mi_cd(const double* vals, const long long* perm,
                                 const long long* ranks, const int* cid, const int* seg,
                                 const double* psi, int F, int n, int n_neighbors, double* part,
                                 int tiles, double* sum, int* m_out, long long ldm,
                                 const int* rowmap, hipStream_t stream) {
  if (F <= 0) return hipSuccess;
  if (n < 2 || n_neighbors < 1 || n_neighbors > cnmf::kMiMaxNeighbors || F > 65535 ||
      tiles != (n + cnmf::kMiThreads - 1) / cnmf::kMiThreads ||
      (m_out != nullptr && rowmap == nullptr))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(cnmf::mi_cd_kernel, dim3(tiles, F), dim3(cnmf::kMiThreads), 0, stream,
                     vals, perm, ranks, cid, seg, psi, n, n_neighbors, part, tiles, m_out, ldm,
                     rowmap);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(cnmf::mi_cd_sum_kernel, dim3(F), dim3(64), 0, stream, part, tiles, sum);
  return hipGetLastError();
}
