// Kernel template of the split-precision GEMM (see gemm_planes.hip for the method) and its
// launcher, shared by the instantiation units gemm_planes.hip (tile variants 0-5) and
// gemm_planes_b2.hip / gemm_planes_b3.hip (the NI != 4 tile family).
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

namespace cnmf {

typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4v __attribute__((ext_vector_type(4)));

struct PlaneGemmParams {
  const unsigned short* A;  // plane p at A + p * a_plane, rows [a_rows][lda] (k contiguous)
  long long lda, a_plane;
  int a_rows;
  const unsigned short* B;  // plane p at B + p * b_plane, rows [b_rows][ldb]
  long long ldb, b_plane;
  int b_rows;
  float* C;                 // [M][ldc]
  long long ldc;
  const float* col_scale;   // optional per-output-column factor
  int M, N, Kd;             // Kd: multiple of BK
  int accumulate;           // C += instead of C =
  int tiles_m, tiles_n;
  int ksplit;               // > 1: workgroup z-slice of k; raw partials to `slab`
  float* slab;              // [ksplit][M][N] partial products (split-K only)
  int raw;                  // 1: raw partials to `slab` even at ksplit 1, and no reduce --
                            // the consuming solve sums them (solve_pipe.hip numer slabs)
  const int* gate;          // optional: *gate == 0 -> every workgroup returns at once (an
                            // online pass enqueued after every replicate had finished)
};

// 16-byte chunk swizzle within a tile row (chunk count CPR): conflict-free ds_read_b128
// for the 16x16x32 fragment pattern (rows lane&15, chunk lane>>4) -- checked against the
// gfx950 ds_read_b128 lane groups.
template <int CPR>
__device__ __forceinline__ int swz(int row) {
  return CPR == 8 ? (row & 7) : ((row >> 1) & 3);
}

__device__ __forceinline__ void glds16(const unsigned short* g, unsigned char* lds) {
  __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)g,
                                   (void __attribute__((address_space(3)))*)lds, 16, 0, 0);
}

// Output tile (16 MI WM) x (16 NI WN): WM x WN waves, each owning MI x NI blocks of 16 x 16.
// The B tile's 16-byte chunks need not divide over the threads (160 rows x 4 chunks over
// 256 threads is 2.5 each): they are dealt to the waves in rounds of 64, the first B_REM
// waves issue one round more than the others, and every wave's vmcnt count is that of ITS
// loads (a wave-uniform branch between two compile-time counts).
template <int PA, int PB, int BK, int WM, int WN, int NS, int MI = 4, int NI = 4>
__global__ __launch_bounds__(64 * WM * WN) void gemm_planes_kernel(PlaneGemmParams p) {
  // gate: read now, tested after the prologue's loads are issued, so its latency hides
  // behind theirs (testing it first cost ~1 % of the headline: every GEMM waited for it)
  const int gate_v = p.gate ? *p.gate : 1;
  constexpr int NW = WM * WN;                 // waves
  constexpr int NT = 64 * NW;                 // threads
  constexpr int WR = 16 * MI, WC = 16 * NI;   // each wave owns a WR x WC output block
  constexpr int BM = WR * WM, BN = WC * WN;
  constexpr int CPR = BK / 8;                 // 16-byte chunks per tile row
  constexpr int A_TILE = BM * BK * 2;         // bytes per plane tile
  constexpr int B_TILE = BN * BK * 2;
  constexpr int STAGE = PA * A_TILE + PB * B_TILE;
  constexpr int A_LD = BM * CPR / NT;         // glds per thread per A plane
  constexpr int B_WCH = BN * CPR / 64;        // B plane tile in wave-rounds of 64 chunks
  constexpr int B_FULL = B_WCH / NW;          // rounds every wave issues
  constexpr int B_REM = B_WCH % NW;           // waves [0, B_REM) issue one more
  constexpr int B_LD = B_FULL + (B_REM ? 1 : 0);
  constexpr int LOADS = PA * A_LD + PB * B_LD;       // of waves [0, B_REM) (all if B_REM = 0)
  constexpr int LOADS_LO = PA * A_LD + PB * B_FULL;  // of the other waves
  static_assert(A_LD * NT == BM * CPR && B_WCH * 64 == BN * CPR, "tile / thread mismatch");
  static_assert(NS >= 2 && NS <= 4, "2..4 stages");
  static_assert((NS >= 4 ? 2 : 1) * LOADS < 64, "vmcnt is a 6-bit counter");
  static_assert(NS * STAGE <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char smem[NS * STAGE];

  // XCD-aware bijective remap; consecutive logical tiles share the M panel (the A
  // operand: three planes, the larger one), so an XCD keeps its A panels in its L2 and
  // streams B
  const int nwg = p.tiles_m * p.tiles_n;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int tn = wg % p.tiles_n, tm = wg / p.tiles_n;
  const int m0 = tm * BM, n0 = tn * BN;
  // k range of this workgroup (split-K slice blockIdx.y)
  const int nk_all = p.Kd / BK;
  const int ks = blockIdx.y;
  const int kb = (int)((long long)nk_all * ks / p.ksplit);
  const int ke = (int)((long long)nk_all * (ks + 1) / p.ksplit);

  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int wm = wave / WN, wn = wave % WN;
  // the wave's share of a ragged B tile, as a scalar (the branches on it are wave-uniform)
  const bool b_more = B_REM > 0 && __builtin_amdgcn_readfirstlane(wave) < B_REM;

  // per-thread global source offsets (elements) of its glds chunks, k excluded (the extra
  // round's offsets of a wave outside it are clamped like any row and never used)
  long long a_off[A_LD], b_off[B_LD > 0 ? B_LD : 1];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const int qd = i * NT + t, row = qd / CPR, pos = qd % CPR;
    const int gr = min(m0 + row, p.a_rows - 1);
    a_off[i] = (long long)gr * p.lda + (pos ^ swz<CPR>(row)) * 8;
  }
#pragma unroll
  for (int i = 0; i < B_LD; ++i) {
    const int qd = i * NT + t, row = qd / CPR, pos = qd % CPR;
    const int gr = min(n0 + row, p.b_rows - 1);
    b_off[i] = (long long)gr * p.ldb + (pos ^ swz<CPR>(row)) * 8;
  }

  auto issue = [&](int stage, int k0) {
    unsigned char* base = smem + stage * STAGE;
#pragma unroll
    for (int pl = 0; pl < PA; ++pl)
#pragma unroll
      for (int i = 0; i < A_LD; ++i)
        glds16(p.A + pl * p.a_plane + a_off[i] + k0,
               base + pl * A_TILE + (i * NT + wave * 64) * 16);
#pragma unroll
    for (int pl = 0; pl < PB; ++pl)
#pragma unroll
      for (int i = 0; i < B_FULL; ++i)
        glds16(p.B + pl * p.b_plane + b_off[i] + k0,
               base + PA * A_TILE + pl * B_TILE + (i * NT + wave * 64) * 16);
    if constexpr (B_REM > 0) {
      if (b_more) {
#pragma unroll
        for (int pl = 0; pl < PB; ++pl)
          glds16(p.B + pl * p.b_plane + b_off[B_FULL] + k0,
                 base + PA * A_TILE + pl * B_TILE + (B_FULL * NT + wave * 64) * 16);
      }
    }
  };
  // wait until at most `stages_left` later stages of THIS wave's loads are outstanding
  auto wait_stages = [&](auto stages_left) {
    constexpr int S = decltype(stages_left)::value;
    if constexpr (B_REM > 0 && S > 0) {
      if (b_more) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S * LOADS) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S * LOADS_LO) : "memory");
    } else {
      asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S * LOADS) : "memory");
    }
  };

  f32x4v acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};

  // NS-stage ring: stage kt+NS-1 is issued right after the barrier that certifies every
  // wave has finished multiplying stage kt-1 (whose slot it refills), so ONE barrier per
  // k-step and NS-1 k-steps of loads in flight behind the MFMAs
#pragma unroll
  for (int s = 0; s < NS - 1; ++s)
    if (kb + s < ke) issue(s, (kb + s) * BK);
  if (gate_v == 0) {   // uniform: nothing to compute; drain the LDS-DMA first
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    return;
  }
  for (int kt = kb; kt < ke; ++kt) {
    const int cur = (kt - kb) % NS;
    // stage kt has landed once at most min(NS-2, ke-1-kt) later stages are outstanding
    const int later = min(NS - 2, ke - 1 - kt);
    if (later >= 2) {
      if constexpr (NS >= 4) wait_stages(std::integral_constant<int, 2>{});
    } else if (later == 1) wait_stages(std::integral_constant<int, 1>{});
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    // this wave's fragment reads of the slot refilled below have returned
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + NS - 1 < ke) issue((kt - kb + NS - 1) % NS, (kt + NS - 1) * BK);
    const unsigned char* As = smem + cur * STAGE;
    const unsigned char* Bs = As + PA * A_TILE;
#pragma unroll
    for (int kk = 0; kk < BK / 32; ++kk) {
      const int c = kk * 4 + (lane >> 4);
      bf16x8 bfr[PB][NI];
#pragma unroll
      for (int j = 0; j < PB; ++j)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) {
          const int row = wn * WC + ni * 16 + (lane & 15);
          bfr[j][ni] = *(const bf16x8*)(Bs + j * B_TILE + row * (BK * 2) +
                                        ((c ^ swz<CPR>(row)) * 16));
        }
      bf16x8 afr[PA][MI];
#pragma unroll
      for (int i = 0; i < PA; ++i)
#pragma unroll
        for (int mi = 0; mi < MI; ++mi) {
          const int row = wm * WR + mi * 16 + (lane & 15);
          afr[i][mi] = *(const bf16x8*)(As + i * A_TILE + row * (BK * 2) +
                                        ((c ^ swz<CPR>(row)) * 16));
        }
#pragma unroll
      for (int mi = 0; mi < MI; ++mi)
#pragma unroll
        for (int ni = 0; ni < NI; ++ni)
#pragma unroll
          for (int i = PA - 1; i >= 0; --i)      // small planes first
#pragma unroll
            for (int j = PB - 1; j >= 0; --j)
              if (i + j <= 2)
                acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(afr[i][mi], bfr[j][ni],
                                                                      acc[mi][ni], 0, 0, 0);
    }
  }

  if (p.ksplit > 1 || p.raw) {   // raw partial tile -> slab ks (reduced in slice order
                                 // by gemm_reduce, or by the consumer when raw)
    float* sl = p.slab + (long long)ks * p.M * p.N;
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int gn = n0 + wn * WC + ni * 16 + (lane & 15);
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int gm = m0 + wm * WR + mi * 16 + (lane >> 4) * 4 + rr;
          if (gm < p.M && gn < p.N) sl[(long long)gm * p.N + gn] = acc[mi][ni][rr];
        }
      }
    return;
  }

  // epilogue: lane holds rows (lane>>4)*4 + r of column lane&15 of each 16x16 block.
  // Accumulating: every old value is loaded (clamped addresses, no per-element branch)
  // before any is used, so the loads are in flight together.
  float sc[NI];
  int gn[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    gn[ni] = n0 + wn * WC + ni * 16 + (lane & 15);
    sc[ni] = p.col_scale ? p.col_scale[min(gn[ni], p.N - 1)] : 1.f;
  }
  const int gm0 = m0 + wm * WR + (lane >> 4) * 4;
  if (p.accumulate) {
    float old[MI][NI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          old[mi][ni][rr] = p.C[(long long)min(gm0 + mi * 16 + rr, p.M - 1) * p.ldc +
                                min(gn[ni], p.N - 1)];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int gm = gm0 + mi * 16 + rr;
          if (gm < p.M && gn[ni] < p.N)
            p.C[(long long)gm * p.ldc + gn[ni]] = old[mi][ni][rr] + acc[mi][ni][rr] * sc[ni];
        }
  } else {
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int gm = gm0 + mi * 16 + rr;
          if (gm < p.M && gn[ni] < p.N)
            p.C[(long long)gm * p.ldc + gn[ni]] = acc[mi][ni][rr] * sc[ni];
        }
  }
}

template <int PA, int PB, int BK, int WM, int WN, int MI = 4, int NI = 4>
static hipError_t launch_gemm(PlaneGemmParams p, int stages, hipStream_t s) {
  constexpr int stage_bytes = (PA * 16 * MI * WM + PB * 16 * NI * WN) * BK * 2;
  if constexpr (BK > 32 && 2 * stage_bytes > 160 * 1024) {
    return launch_gemm<PA, PB, 32, WM, WN, MI, NI>(p, stages, s);   // deep k-step does not fit
  } else if constexpr (2 * stage_bytes > 160 * 1024) {
    return hipErrorInvalidValue;   // 128 x 320 with 3 + 3 planes: the plan never picks it
  } else {
  p.tiles_m = (p.M + 16 * MI * WM - 1) / (16 * MI * WM);
  p.tiles_n = (p.N + 16 * NI * WN - 1) / (16 * NI * WN);
  const dim3 grid(p.tiles_m * p.tiles_n, p.ksplit), block(64 * WM * WN);
  if constexpr (3 * stage_bytes <= 160 * 1024) {
    if (stages >= 3) {
      hipLaunchKernelGGL((gemm_planes_kernel<PA, PB, BK, WM, WN, 3, MI, NI>), grid, block, 0, s,
                         p);
      return hipGetLastError();
    }
  }
  hipLaunchKernelGGL((gemm_planes_kernel<PA, PB, BK, WM, WN, 2, MI, NI>), grid, block, 0, s, p);
  return hipGetLastError();
  }
}

// return FN<PA, PB>(args) for the runtime plane counts (pa 2..3, pb 1..3)
#define CNMF_GEMM_DISPATCH_PLANES(FN, pa, pb, ...)                         \
  switch ((pa) * 4 + (pb)) {                                               \
    case 9: return FN<2, 1>(__VA_ARGS__);                                  \
    case 10: return FN<2, 2>(__VA_ARGS__);                                 \
    case 11: return FN<2, 3>(__VA_ARGS__);                                 \
    case 13: return FN<3, 1>(__VA_ARGS__);                                 \
    case 14: return FN<3, 2>(__VA_ARGS__);                                 \
    default: return FN<3, 3>(__VA_ARGS__);                                 \
  }

// tile variants 6-7 (gemm_planes_b2.hip) and 8-9 (gemm_planes_b3.hip)
hipError_t launch_gemm_wide(int pa, int pb, int v, const PlaneGemmParams& p, int stages, int bk,
                            hipStream_t s);
hipError_t launch_gemm_narrow(int pa, int pb, int v, const PlaneGemmParams& p, int stages, int bk,
                              hipStream_t s);

}  // namespace cnmf
