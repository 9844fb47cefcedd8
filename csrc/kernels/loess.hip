// Local polynomial regression (LOESS, tricube weights, degree 1 or 2) of B independent
// series laid end to end, as ops/reference.py ``loess`` defines it (docs/ARCHITECTURE.md
// "LOESS").  The host sorts every series; series b occupies [offsets[b], offsets[b + 1]) of
// xs / ys and uses a window of ks[b] = min(m, max(degree + 1, ceil(span * m))) points.
//
// loess_windows_kernel, one thread per point i of a series of m points with window k: the
// window start is the first lo in [0, m - k] at which
//     xs[lo + k] - xs[i] < xs[i] - xs[lo]
// is false (lo = m - k counts as false).  The left side grows and the right side shrinks
// with lo, so the predicate is monotone and a bisection finds the point the sliding loop of
// models/pp.py ``loess_fit`` stops at.  Starts are positions inside the series.
//
// loess_fit_kernel<DEGREE>, one wave per point and four waves per workgroup: the lanes
// stride the window [s, s + k) of the sorted series in coalesced order (the two arrays are
// 16 bytes per point and stay in L2), each lane adds its share of S_p = sum w d^p
// (p <= 2 DEGREE) and T_p = sum w d^p y (p <= DEGREE) in window order, and a butterfly folds
// the 64 lane sums in a fixed order, so every run gives the same bits.  h is the larger
// distance to the two window ends (the window is sorted), times 1.0000001, or 1 when it is
// 0; w = max(1 - (|d| / h)^3, 0)^3.  The wave then solves (S_{a+b} + 1e-10 I) c = T by
// Gaussian elimination with partial pivoting and lane 0 stores c_0 at the point's sorted
// position.  No atomics, no LDS, nothing of size n * k.
//
// Every loop has a fixed trip bound and every index is clamped into its series.
#include <hip/hip_runtime.h>

#include "common.h"

namespace cnmf {

constexpr int kLoessThreads = 256;
constexpr int kLoessWaves = kLoessThreads / 64;

// the series of global position i: the first b in [0, B) with offsets[b + 1] > i
__device__ __forceinline__ int loess_series(const int* __restrict__ offsets, int B, int i) {
  int a = 0, b = B - 1;
  for (int it = 0; it < 32; ++it) {
    if (a >= b) break;
    const int mid = a + ((b - a) >> 1);
    if (offsets[mid + 1] > i) b = mid; else a = mid + 1;
  }
  return a;
}

__global__ __launch_bounds__(kLoessThreads) void loess_windows_kernel(
    const double* __restrict__ xs, const int* __restrict__ offsets, const int* __restrict__ ks,
    int B, int n, int* __restrict__ starts) {
  const long long gi = (long long)blockIdx.x * kLoessThreads + threadIdx.x;
  if (gi >= n) return;
  const int i = (int)gi;
  const int b = loess_series(offsets, B, i);
  const int base = max(offsets[b], 0);
  const int m = min(offsets[b + 1], n) - base;
  const int li = i - base;
  if (m <= 0 || li < 0 || li >= m) return;
  const int k = min(max(ks[b], 1), m);
  const double* __restrict__ x = xs + base;
  const double xi = x[li];
  int lo = 0, hi = m - k;                       // the answer lies in [lo, hi]
  for (int it = 0; it < 32; ++it) {
    if (lo >= hi) break;
    const int mid = lo + ((hi - lo) >> 1);      // mid < m - k, so mid + k < m
    if ((x[mid + k] - xi) < (xi - x[mid])) lo = mid + 1; else hi = mid;
  }
  starts[i] = lo;
}

template <int DEGREE>
__global__ __launch_bounds__(kLoessThreads) void loess_fit_kernel(
    const double* __restrict__ xs, const double* __restrict__ ys,
    const int* __restrict__ offsets, const int* __restrict__ ks,
    const int* __restrict__ starts, int B, int n, double* __restrict__ fitted) {
  constexpr int NS = 2 * DEGREE + 1, NT = DEGREE + 1;
  const int lane = threadIdx.x & 63;
  const long long gi = (long long)blockIdx.x * kLoessWaves + (threadIdx.x >> 6);
  if (gi >= n) return;                          // wave-uniform
  const int i = (int)gi;
  const int b = loess_series(offsets, B, i);
  const int base = max(offsets[b], 0);
  const int m = min(offsets[b + 1], n) - base;
  const int li = i - base;
  if (m <= 0 || li < 0 || li >= m) return;
  const int k = min(max(ks[b], 1), m);
  const int s = min(max(starts[i], 0), m - k);
  const double* __restrict__ x = xs + base + s;
  const double* __restrict__ y = ys + base + s;
  const double xi = xs[base + li];
  double h = fmax(xi - x[0], x[k - 1] - xi);
  h = h > 0.0 ? h * 1.0000001 : 1.0;
  double S[NS], T[NT];
#pragma unroll
  for (int p = 0; p < NS; ++p) S[p] = 0.0;
#pragma unroll
  for (int p = 0; p < NT; ++p) T[p] = 0.0;
  for (int j = lane; j < k; j += 64) {
    const double d = x[j] - xi;
    const double yj = y[j];
    const double r = fabs(d) / h;
    const double u = fmax(1.0 - r * r * r, 0.0);
    double pw = u * u * u;                      // w d^p
#pragma unroll
    for (int p = 0; p < NS; ++p) {
      S[p] += pw;
      if (p < NT) T[p] += pw * yj;
      pw *= d;
    }
  }
#pragma unroll
  for (int p = 0; p < NS; ++p) S[p] = wave_sum(S[p]);
#pragma unroll
  for (int p = 0; p < NT; ++p) T[p] = wave_sum(T[p]);
  // every lane holds the same sums; the solve is wave-uniform
  double A[NT][NT + 1];
#pragma unroll
  for (int a = 0; a < NT; ++a) {
#pragma unroll
    for (int c = 0; c < NT; ++c) A[a][c] = S[a + c] + (a == c ? 1e-10 : 0.0);
    A[a][NT] = T[a];
  }
#pragma unroll
  for (int c = 0; c < NT; ++c) {
    // partial pivoting: the first row of the largest |A[r][c]|, r >= c, swapped into row c
#pragma unroll
    for (int r = c + 1; r < NT; ++r) {
      if (fabs(A[r][c]) > fabs(A[c][c])) {
#pragma unroll
        for (int q = 0; q <= NT; ++q) {
          const double t = A[c][q];
          A[c][q] = A[r][q];
          A[r][q] = t;
        }
      }
    }
#pragma unroll
    for (int r = c + 1; r < NT; ++r) {
      const double f = A[r][c] / A[c][c];
#pragma unroll
      for (int q = c; q <= NT; ++q) A[r][q] -= f * A[c][q];
    }
  }
  double coef[NT];
#pragma unroll
  for (int a = NT - 1; a >= 0; --a) {
    double v = A[a][NT];
#pragma unroll
    for (int c = a + 1; c < NT; ++c) v -= A[a][c] * coef[c];
    coef[a] = v / A[a][a];
  }
  if (lane == 0) fitted[i] = coef[0];
}

static bool loess_args_ok(int B, int n) { return B >= 1 && n >= 0; }

}  // namespace cnmf

// xs (n) the series sorted and laid end to end; offsets (B + 1) with offsets[0] = 0,
// non-decreasing, offsets[B] = n; ks (B) the window of every series, 1 <= ks[b] <= its
// length; starts (n) receives the window start of every point inside its series.
extern "C" hipError_t cnmf_loess_windows(const double* xs, const int* offsets, const int* ks,
                                         int B, int n, int* starts, hipStream_t stream) {
  if (!cnmf::loess_args_ok(B, n)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((long long)n + cnmf::kLoessThreads - 1) /
                                     cnmf::kLoessThreads);
  hipLaunchKernelGGL(cnmf::loess_windows_kernel, dim3(blocks), dim3(cnmf::kLoessThreads), 0,
                     stream, xs, offsets, ks, B, n, starts);
  return hipGetLastError();
}

// fitted (n) receives the fitted value of every point at its sorted position
extern "C" hipError_t cnmf_loess_fit(const double* xs, const double* ys, const int* offsets,
                                     const int* ks, const int* starts, int B, int n, int degree,
                                     double* fitted, hipStream_t stream) {
  if (!cnmf::loess_args_ok(B, n) || (degree != 1 && degree != 2)) return hipErrorInvalidValue;
  if (n == 0) return hipSuccess;
  const unsigned blocks = (unsigned)(((long long)n + cnmf::kLoessWaves - 1) /
                                     cnmf::kLoessWaves);
  if (degree == 1)
    hipLaunchKernelGGL(cnmf::loess_fit_kernel<1>, dim3(blocks), dim3(cnmf::kLoessThreads), 0,
                       stream, xs, ys, offsets, ks, starts, B, n, fitted);
  else
    hipLaunchKernelGGL(cnmf::loess_fit_kernel<2>, dim3(blocks), dim3(cnmf::kLoessThreads), 0,
                       stream, xs, ys, offsets, ks, starts, B, n, fitted);
  return hipGetLastError();
}
