// Split-precision fp32 GEMM on the bf16 matrix cores (the
// data-side products of every online NMF step, numer = W X_c^T and B += H_c^T X_c).
//
// gfx950 has no xf32/TF32 MFMA: fp32 operands run at the vector rate (157 TF), 1/16 of
// bf16 MFMA (2.5 PF).  An fp32 value splits EXACTLY into three bf16 planes
// (v = hi + mid + lo: 8 + 8 + 8 mantissa bits, each residual exact in fp32), and a
// bf16 x bf16 product is exact in the fp32 accumulator.  So
//
//     C = sum over plane pairs (i, j) with i + j <= 2 of  A_i . B_j^T      (fp32 accumulate)
//
// reproduces the fp32 GEMM to fp32 rounding (the dropped pairs are < 2^-24 relative).
// With TWO A planes (PA = 2: hi + mid, |v - hi - mid| <= 2^-16 |v|) the product error is
// <= 2^-16 sum|a b| -- inside the standard fp32 GEMM bound n 2^-24 sum|a b| for every
// reduction length n >= 256, and from n ~ 1000 on measured below hipBLASLt's fp32 GEMM
// error (tests:
// test_gemm_two_a_planes_within_fp32_library_error); the engine uses it for k >= 1024.
// The cNMF data matrix is counts / per-gene std: with the per-gene unit folded into the
// OTHER operand (A's columns for numer, C's columns for B) the count matrix is held
// exactly by ONE bf16 plane (counts <= 256) or two (< 65536), so the product costs 3 (or
// 5) bf16 MFMAs instead of one fp32 MFMA of 16x the cycles.  The operand planes are
// produced once per update by ``split_planes_kernel`` (X: once per factorisation).
//
// Tiling: 128 x 128 output tile per 256-thread workgroup (2 x 2 waves, 64 x 64 each,
// 4 x 4 accumulators of v_mfma_f32_16x16x32_bf16), BK-deep k-steps staged global -> LDS
// by LDS-DMA (global_load_lds_dwordx4, 16 B per lane) into two buffers: step k+1 is in
// flight while step k is multiplied (counted vmcnt + raw s_barrier, never a vmcnt(0)
// inside the loop -- cdna_hip_programming.md §5 "Pipelining across barriers").  LDS rows
// are 16-byte-chunk XOR-swizzled on the SOURCE address (glds writes lane-linear), which
// makes the ds_read_b128 fragment reads conflict-free.  Workgroup ids are remapped so a
// run of consecutive tiles shares one XCD's L2 (T1).  Rows of A / B beyond the matrix
// are clamped (valid memory, results discarded); the k range must be padded to BK with
// zeros in A (the caller's plane buffers are).  The kernel template is gemm_planes.h: the
// wave block is MI x NI blocks of 16 x 16, so tiles are 16 MI WM x 16 NI WN (table below).
#include "gemm_planes.h"

namespace cnmf {

__device__ __forceinline__ unsigned short f2bf_rn(float f) {
  unsigned u = __float_as_uint(f);
  u += 0x7FFFu + ((u >> 16) & 1u);  // round to nearest even (finite inputs)
  return (unsigned short)(u >> 16);
}
__device__ __forceinline__ float bf2f(unsigned short h) {
  return __uint_as_float((unsigned)h << 16);
}

// S (rows x cols, row stride lds) [* col_mul] -> nplanes bf16 planes [rows][ldp], plane
// stride `plane`; columns [cols, cols_pad) are written as zeros (k padding of the GEMM).
// Each thread converts 4 consecutive columns.
__global__ void split_planes_kernel(const float* __restrict__ S, long long lds, int rows,
                                    int cols, int cols_pad, const float* __restrict__ col_mul,
                                    unsigned short* __restrict__ P, long long ldp,
                                    long long plane, int nplanes) {
  const int c4 = cols_pad / 4;
  const long long total = (long long)rows * c4;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    const int r = (int)(i / c4);
    const int c = (int)(i - (long long)r * c4) * 4;
    unsigned short h[3][4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int cc = c + e;
      float v = 0.f;
      if (cc < cols) {
        v = S[(long long)r * lds + cc];
        if (col_mul) v *= col_mul[cc];
      }
      const unsigned short h0 = f2bf_rn(v);
      const float r1 = v - bf2f(h0);
      const unsigned short h1 = f2bf_rn(r1);
      const float r2 = r1 - bf2f(h1);
      h[0][e] = h0;
      h[1][e] = h1;
      h[2][e] = f2bf_rn(r2);
    }
    for (int pl = 0; pl < nplanes; ++pl) {
      uint2 w;
      w.x = (unsigned)h[pl][0] | ((unsigned)h[pl][1] << 16);
      w.y = (unsigned)h[pl][2] | ((unsigned)h[pl][3] << 16);
      *(uint2*)(P + pl * plane + (long long)r * ldp + c) = w;
    }
  }
}

// C (+)= col_scale * sum_s slab[s] in slice order (deterministic split-K reduction)
__global__ void gemm_reduce_kernel(const float* __restrict__ slab, int ksplit, int M, int N,
                                   float* __restrict__ C, long long ldc,
                                   const float* __restrict__ col_scale, int accumulate,
                                   const int* gate) {
  // (the gate is not tested here: a reduce of a skipped product writes an output no
  // replicate reads, and waiting for the flag cost more than the rare skip saves)
  (void)gate;
  const long long total = (long long)M * N;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total;
       i += (long long)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int s = 0; s < ksplit; ++s) v += slab[(long long)s * total + i];
    const int m = (int)(i / N), n = (int)(i - (long long)m * N);
    if (col_scale) v *= col_scale[n];
    float* cp = C + (long long)m * ldc + n;
    *cp = accumulate ? *cp + v : v;
  }
}

// tile variants: 0 = 128x128 (4 waves), 1 = 128x256 (8 waves), 2 = 256x128 (8 waves),
// 3 = 64x128 (2 waves), 4 = 64x128 (4 waves of 32 x 64: twice the waves per output),
// 5 = 128x128 (8 waves of 32 x 64); 6-9 (wave blocks of NI != 4 column blocks) are
// instantiated in gemm_planes_b2.hip / gemm_planes_b3.hip
template <int PA, int PB, int BK>
static hipError_t launch_variant_bk(int v, const PlaneGemmParams& p, int stages, hipStream_t s) {
  switch (v) {
    case 0: return launch_gemm<PA, PB, BK, 2, 2>(p, stages, s);
    case 1: return launch_gemm<PA, PB, BK, 2, 4>(p, stages, s);
    case 2: return launch_gemm<PA, PB, BK, 4, 2>(p, stages, s);
    case 4: return launch_gemm<PA, PB, BK, 2, 2, 2>(p, stages, s);   // 64 x 128, 4 waves
    case 5: return launch_gemm<PA, PB, BK, 4, 2, 2>(p, stages, s);   // 128 x 128, 8 waves
    default: return launch_gemm<PA, PB, BK, 1, 2>(p, stages, s);
  }
}

// k-step depth: 64 (two MFMA k-steps per LDS stage and barrier: the second step's
// fragment reads overlap the first step's MFMAs) where it fits and divides Kd, else 32
template <int PA, int PB>
static hipError_t launch_variant(int v, const PlaneGemmParams& p, int stages, int bk,
                                 hipStream_t s) {
  if (bk >= 64 && p.Kd % 64 == 0) return launch_variant_bk<PA, PB, 64>(v, p, stages, s);
  return launch_variant_bk<PA, PB, 32>(v, p, stages, s);
}

}  // namespace cnmf

// k granularity the caller pads the planes to (a multiple of every k-step depth)
extern "C" int cnmf_gemm_planes_bk(int pb) { return 64; }

// Tile tables: rows of (M-tile, N-tile) per variant, for the host heuristics.
extern "C" int cnmf_gemm_planes_tile(int v, int which) {
  static const int tm[10] = {128, 128, 256, 64, 64, 128, 128, 128, 128, 128};
  static const int tn[10] = {128, 256, 128, 128, 128, 128, 160, 320, 64, 32};
  return (v < 0 || v > 9) ? 0 : (which == 0 ? tm[v] : tn[v]);
}

extern "C" hipError_t cnmf_gemm_planes(const unsigned short* A, long long lda, long long a_plane,
                                       int a_rows, const unsigned short* B, long long ldb,
                                       long long b_plane, int b_rows, float* C, long long ldc,
                                       const float* col_scale, int M, int N, int Kd, int pa,
                                       int pb, int accumulate, int variant, int ksplit,
                                       float* slab, int stages, int kstep, int raw,
                                       const int* gate, hipStream_t stream) {
  if (M <= 0 || N <= 0) return hipSuccess;
  if (raw && !slab) return hipErrorInvalidValue;
  const int bk = 32;   // smallest k-step depth: Kd must be a multiple of it
  if (pa < 2 || pa > 3 || pb < 1 || pb > 3 || Kd <= 0 || Kd % bk || lda % 8 || ldb % 8 ||
      a_plane % 8 || b_plane % 8 || a_rows < 1 || b_rows < 1 || variant < 0 || variant > 9 ||
      ksplit < 1 || ksplit > Kd / (kstep >= 64 && Kd % 64 == 0 ? 64 : bk) ||
      (ksplit > 1 && !slab))
    return hipErrorInvalidValue;
  cnmf::PlaneGemmParams p;
  p.A = A; p.lda = lda; p.a_plane = a_plane; p.a_rows = a_rows;
  p.B = B; p.ldb = ldb; p.b_plane = b_plane; p.b_rows = b_rows;
  p.C = C; p.ldc = ldc; p.col_scale = col_scale;
  p.M = M; p.N = N; p.Kd = Kd; p.accumulate = accumulate;
  p.ksplit = ksplit; p.slab = slab; p.raw = raw ? 1 : 0; p.gate = gate;
  hipError_t e;
  if (variant >= 8) e = cnmf::launch_gemm_narrow(pa, pb, variant, p, stages, kstep, stream);
  else if (variant >= 6) e = cnmf::launch_gemm_wide(pa, pb, variant, p, stages, kstep, stream);
  else switch (pa * 4 + pb) {
    case 9: e = cnmf::launch_variant<2, 1>(variant, p, stages, kstep, stream); break;
    case 10: e = cnmf::launch_variant<2, 2>(variant, p, stages, kstep, stream); break;
    case 11: e = cnmf::launch_variant<2, 3>(variant, p, stages, kstep, stream); break;
    case 13: e = cnmf::launch_variant<3, 1>(variant, p, stages, kstep, stream); break;
    case 14: e = cnmf::launch_variant<3, 2>(variant, p, stages, kstep, stream); break;
    default: e = cnmf::launch_variant<3, 3>(variant, p, stages, kstep, stream); break;
  }
  if (e != hipSuccess || ksplit == 1 || raw) return e;
  const long long total = (long long)M * N;
  long long blocks = (total + 255) / 256;
  if (blocks > 4096) blocks = 4096;
  hipLaunchKernelGGL(cnmf::gemm_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, slab,
                     ksplit, M, N, C, ldc, col_scale, accumulate, gate);
  return hipGetLastError();
}

extern "C" hipError_t cnmf_split_planes(const float* S, long long lds, int rows, int cols,
                                        int cols_pad, const float* col_mul, unsigned short* P,
                                        long long ldp, long long plane, int nplanes,
                                        hipStream_t stream) {
  if (rows <= 0 || cols_pad <= 0) return hipSuccess;
  if (cols_pad % 4 || ldp % 4 || cols > cols_pad || nplanes < 1 || nplanes > 3)
    return hipErrorInvalidValue;
  const long long total = (long long)rows * (cols_pad / 4);
  long long blocks = (total + 255) / 256;
  if (blocks > 8192) blocks = 8192;
  hipLaunchKernelGGL(cnmf::split_planes_kernel, dim3((unsigned)blocks), dim3(256), 0, stream, S,
                     lds, rows, cols, cols_pad, col_mul, P, ldp, plane, nplanes);
  return hipGetLastError();
}
