// Data-side products of the online NMF step on a SPARSE data matrix held as tiles of its
// non-zeros (models.nmf_base.SparseTilesX): the same split-precision product as
// gemm_planes.hip -- the sum over plane pairs (i, j), i + j <= 2, of A_i . B_j^T on
// v_mfma_f32_16x16x32_bf16 -- with the B tile of every k-step built in LDS from the
// entries instead of copied from dense planes.
//
// Format.  X (N cells x G genes) is cut into tiles of 64 cells x 64 genes, row-tile major
// (tile id = (cell / 64) * ceil(G / 64) + gene / 64); the entries of a tile are contiguous
// and tile_ptr (64-bit, one per tile plus one) delimits them.  An entry is one 32-bit
// word: bits 0-15 the bf16 pattern of value plane 0, bits 16-21 the local gene, bits 22-27
// the local cell.  Planes 1 and 2 (counts above 256, non-count data) are parallel 16-bit
// arrays.  One copy serves both products:
//
//   side n:  C[:M, cell - r0]  = A . X[r0:r1, :]^T   k = gene,      LDS row = local cell
//   side s:  C[:M, gene]     (+)= A . X[r0:r1, :]    k = cell - r0, LDS row = local gene
//
// Chunk starts are not multiples of the tile height (5000 = 78 * 64 + 8).  Side s walks A
// in 64-deep steps from r0 and fills each B tile from the (up to two) storage row tiles
// the step straddles, dropping entries whose cell is outside the step or beyond r1; r0
// may therefore be ANY row (A's k offsets are multiples of 64 whatever r0 is).  Side n
// gives each workgroup one storage row tile -- so a k-step's B tile is exactly one stored
// tile -- and masks the output columns whose cell is outside [r0, r1).
//
// Workgroup: 128 x 64 output tile, 4 waves stacked over M (32 rows x 64 columns each, 2 x 4
// accumulators), 64-deep k-steps, two LDS stages.  A arrives by LDS-DMA exactly as in
// gemm_planes.h (source-swizzled 16-byte chunks, lane-linear destination).  LDS-DMA
// writes wave-uniform base + lane * 16, not a per-lane scatter, so B cannot use it: the B
// tile of the next step is zero-filled (16-byte stores), then -- after a barrier, because
// any thread's entry may land in any thread's zeroed chunk -- the 2-byte values are
// scattered (ds_write_b16, into the same swizzled layout the fragment reads expect), and
// the barrier that opens the next step publishes them.  Two barriers per k-step; the
// MFMAs of the step's two halves sit on either side of the second one.  The first two
// entries a thread scatters are loaded two k-steps ahead and held in registers; a tile
// of more than 512 entries takes the rest in a loop of four loads, then four stores (a
// full tile: 16 entries per thread).
//
// Deterministic: no k split and no atomics -- one workgroup owns an output tile and sums
// its k-steps in order.  Two entries never share an LDS element (the builder emits each
// (cell, gene) once), so the scatter order does not matter.
#include "gemm_planes.h"

namespace cnmf {

struct TileGemmParams {
  const unsigned short* A;   // plane p at A + p * a_plane, rows [a_rows][lda], k contiguous
  long long lda, a_plane;
  int a_rows;
  const unsigned* ent;            // entry words (>= 1 element even when nnz = 0)
  const unsigned short* v1;       // value plane 1 / 2 per entry (PB >= 2 / 3)
  const unsigned short* v2;
  const long long* tile_ptr;      // [ntr * ntg + 1]
  long long nnz;
  int ntr, ntg;                   // row tiles, gene tiles
  float* C;
  long long ldc;
  const float* col_scale;
  int M, N;                       // output rows, output columns (r1 - r0 or G)
  int r0, r1;
  int nk;                         // k-steps
  int accumulate;
  int tiles_m, tiles_n;
  const int* gate;
};

template <int SIDE, int PA, int PB>
__global__ __launch_bounds__(256) void gemm_tiles_kernel(TileGemmParams p) {
  const int gate_v = p.gate ? *p.gate : 1;
  constexpr int BK = 64, NT = 256, MI = 2, NI = 4;
  constexpr int BM = 128, BN = 64, CPR = 8;
  constexpr int A_TILE = BM * BK * 2, B_TILE = BN * BK * 2;
  constexpr int STAGE = PA * A_TILE + PB * B_TILE;
  constexpr int A_LD = BM * CPR / NT;          // glds per thread per A plane
  constexpr int B_ZF = B_TILE / 16 / NT;       // 16-byte zero stores per thread per plane
  constexpr int NSEG = SIDE == 0 ? 1 : 2;      // storage tiles a k-step's B tile draws on
  constexpr int E0 = 2;                        // entries per thread and segment held in
                                               // registers across the mid-step barrier
  static_assert(2 * STAGE <= 160 * 1024, "LDS");
  __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE];

  // XCD-aware bijective remap, as gemm_planes_kernel: consecutive tiles share the A panel
  const int nwg = p.tiles_m * p.tiles_n;
  const int bid = blockIdx.x;
  const int xcd = bid & 7, q = nwg >> 3, r = nwg & 7;
  const int wg = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  const int tn = wg % p.tiles_n, tm = wg / p.tiles_n;
  const int m0 = tm * BM;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int rt0 = p.r0 >> 6;                   // first storage row tile of the range
  const int d = p.r0 & 63;                     // side s: offset of a k-step in its row tile
  const int nk = p.nk;

  long long a_off[A_LD];
#pragma unroll
  for (int i = 0; i < A_LD; ++i) {
    const int qd = i * NT + t, row = qd / CPR, pos = qd % CPR;
    const int gr = min(m0 + row, p.a_rows - 1);
    a_off[i] = (long long)gr * p.lda + (pos ^ swz<CPR>(row)) * 8;
  }
  auto issue_a = [&](int stage, int k0) {
    unsigned char* base = smem + stage * STAGE;
#pragma unroll
    for (int pl = 0; pl < PA; ++pl)
#pragma unroll
      for (int i = 0; i < A_LD; ++i)
        glds16(p.A + pl * p.a_plane + a_off[i] + k0,
               base + pl * A_TILE + (i * NT + wave * 64) * 16);
  };
  auto zero_b = [&](int stage) {
    unsigned char* Bn = smem + stage * STAGE + PA * A_TILE;
#pragma unroll
    for (int i = 0; i < PB * B_ZF; ++i)
      *(uint4*)(Bn + (i * NT + t) * 16) = uint4{0u, 0u, 0u, 0u};
  };

  // entry ranges [beg, end) of the storage tiles behind k-step kt (wave-uniform)
  struct Seg { long long beg[NSEG], end[NSEG]; };
  auto seg_of = [&](int kt) {
    Seg s;
#pragma unroll
    for (int g = 0; g < NSEG; ++g) {
      const int rt = SIDE == 0 ? rt0 + tn : rt0 + kt + g;
      const int gt = SIDE == 0 ? kt : tn;
      const bool live = kt < nk && rt < p.ntr && gt < p.ntg && (g == 0 || d != 0);
      const long long ti = live ? (long long)rt * p.ntg + gt : 0;
      const long long b = p.tile_ptr[ti], e = p.tile_ptr[ti + 1];
      s.beg[g] = live ? b : 0;
      s.end[g] = live ? e : 0;
    }
    return s;
  };
  // one entry -> its 2-byte element(s) of the B tile of `stage` (k-step kt, segment g)
  auto put = [&](int stage, int kt, int g, unsigned w, unsigned short x1, unsigned short x2) {
    const int lr = (w >> 22) & 63, lc = (w >> 16) & 63;
    int row, k;
    bool ok = true;
    if (SIDE == 0) {
      row = lr; k = lc;
    } else {
      row = lc;
      k = lr - d + 64 * g;                                   // cell - (r0 + 64 kt)
      ok = (unsigned)k < 64u && p.r0 + 64 * kt + k < p.r1;
    }
    if (ok) {
      unsigned char* at = smem + stage * STAGE + PA * A_TILE + row * (BK * 2) +
                          (((k >> 3) ^ swz<CPR>(row)) * 16) + (k & 7) * 2;
      *(unsigned short*)at = (unsigned short)(w & 0xFFFFu);
      if (PB >= 2) *(unsigned short*)(at + B_TILE) = x1;
      if (PB >= 3) *(unsigned short*)(at + 2 * B_TILE) = x2;
    }
  };
  struct Held { unsigned w[NSEG][E0]; unsigned short x1[NSEG][E0], x2[NSEG][E0]; };
  const long long last = p.nnz > 0 ? p.nnz - 1 : 0;
  auto preload = [&](const Seg& s) {
    Held h;
#pragma unroll
    for (int g = 0; g < NSEG; ++g)
#pragma unroll
      for (int i = 0; i < E0; ++i) {
        const long long e = min(s.beg[g] + t + i * NT, last);     // clamped: always valid
        h.w[g][i] = p.ent[e];
        h.x1[g][i] = PB >= 2 ? p.v1[e] : (unsigned short)0;
        h.x2[g][i] = PB >= 3 ? p.v2[e] : (unsigned short)0;
      }
    return h;
  };
  auto scatter = [&](int stage, int kt, const Seg& s, const Held& h) {
#pragma unroll
    for (int g = 0; g < NSEG; ++g) {
#pragma unroll
      for (int i = 0; i < E0; ++i)
        if (s.beg[g] + t + i * NT < s.end[g]) put(stage, kt, g, h.w[g][i], h.x1[g][i], h.x2[g][i]);
      // the rest of a tile of more than E0 * NT entries, four loads in flight at a time
      for (long long e0 = s.beg[g] + t + E0 * NT; e0 < s.end[g]; e0 += 4 * NT) {
        unsigned w[4];
        unsigned short x1[4], x2[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const long long e = min(e0 + j * NT, last);
          w[j] = p.ent[e];
          x1[j] = PB >= 2 ? p.v1[e] : (unsigned short)0;
          x2[j] = PB >= 3 ? p.v2[e] : (unsigned short)0;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (e0 + j * NT < s.end[g]) put(stage, kt, g, w[j], x1[j], x2[j]);
      }
    }
  };

  f32x4v acc[MI][NI];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NI; ++j) acc[i][j] = f32x4v{0.f, 0.f, 0.f, 0.f};

  auto compute = [&](int stage, auto kk_c) {
    constexpr int kk = decltype(kk_c)::value;
    const unsigned char* As = smem + stage * STAGE;
    const unsigned char* Bs = As + PA * A_TILE;
    const int c = kk * 4 + (lane >> 4);
    bf16x8 bfr[PB][NI];
#pragma unroll
    for (int j = 0; j < PB; ++j)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni) {
        const int row = ni * 16 + (lane & 15);
        bfr[j][ni] = *(const bf16x8*)(Bs + j * B_TILE + row * (BK * 2) +
                                      ((c ^ swz<CPR>(row)) * 16));
      }
    bf16x8 afr[PA][MI];
#pragma unroll
    for (int i = 0; i < PA; ++i)
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        const int row = wave * 32 + mi * 16 + (lane & 15);
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
  };

  // prologue: stage 0 of k-step 0.  Entries are fetched TWO k-steps ahead of their
  // scatter (s1 / h1: step kt+1, s2: step kt+2), so the loads issued in one step are
  // first needed after the next step's opening wait
  Seg cur_s = seg_of(0);
  Seg s1 = seg_of(1);
  Seg s2 = seg_of(2);
  Held h1;
  {
    Held h = preload(cur_s);
    h1 = preload(s1);
    issue_a(0, 0);
    if (gate_v == 0) {   // uniform: nothing to compute; drain the LDS-DMA first
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      return;
    }
    zero_b(0);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    scatter(0, 0, cur_s, h);
  }
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1, nxt = cur ^ 1;
    // stage cur is complete (this wave's LDS-DMA and scatter), and this wave's fragment
    // reads of stage nxt (k-step kt-1) have returned; the barrier makes that true of all
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    const bool more = kt + 1 < nk;
    const Held h2 = preload(s2);      // (a dead segment loads one clamped, valid entry)
    const Seg s3 = seg_of(kt + 3);
    if (more) {
      issue_a(nxt, (kt + 1) * BK);
      zero_b(nxt);
    }
    compute(cur, std::integral_constant<int, 0>{});
    // every wave's zero-fill of stage nxt has landed before any entry is scattered into it
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    asm volatile("" ::: "memory");
    if (more) scatter(nxt, kt + 1, s1, h1);
    compute(cur, std::integral_constant<int, 1>{});
    s1 = s2;
    s2 = s3;
    h1 = h2;
  }

  // epilogue, as gemm_planes_kernel; output column = col0 + the tile's local column, and
  // side n's col0 is negative when the range starts inside this storage row tile
  const int col0 = SIDE == 0 ? (rt0 + tn) * 64 - p.r0 : tn * 64;
  float sc[NI];
  int gn[NI];
  bool okc[NI];
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    gn[ni] = col0 + ni * 16 + (lane & 15);
    okc[ni] = gn[ni] >= 0 && gn[ni] < p.N;
    sc[ni] = p.col_scale ? p.col_scale[max(0, min(gn[ni], p.N - 1))] : 1.f;
  }
  const int gm0 = m0 + wave * 32 + (lane >> 4) * 4;
  if (p.accumulate) {
    float old[MI][NI][4];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
          old[mi][ni][rr] = p.C[(long long)min(gm0 + mi * 16 + rr, p.M - 1) * p.ldc +
                                max(0, min(gn[ni], p.N - 1))];
#pragma unroll
    for (int mi = 0; mi < MI; ++mi)
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
          const int gm = gm0 + mi * 16 + rr;
          if (gm < p.M && okc[ni])
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
          if (gm < p.M && okc[ni])
            p.C[(long long)gm * p.ldc + gn[ni]] = acc[mi][ni][rr] * sc[ni];
        }
  }
}

template <int SIDE, int PA, int PB>
static hipError_t launch_tiles(const TileGemmParams& p, hipStream_t s) {
  hipLaunchKernelGGL((gemm_tiles_kernel<SIDE, PA, PB>), dim3(p.tiles_m * p.tiles_n), dim3(256), 0,
                     s, p);
  return hipGetLastError();
}
template <int PA, int PB>
static hipError_t launch_tiles_side(int side, const TileGemmParams& p, hipStream_t s) {
  return side == 0 ? launch_tiles<0, PA, PB>(p, s) : launch_tiles<1, PA, PB>(p, s);
}
static hipError_t launch_tiles_planes(int pa, int pb, int side, const TileGemmParams& p,
                                      hipStream_t s) {
  CNMF_GEMM_DISPATCH_PLANES(launch_tiles_side, pa, pb, side, p, s)
}

}  // namespace cnmf

// side 0 = n (C[:M, :r1-r0] = A . X[r0:r1]^T, A's k = gene, >= ntg * 64 deep),
// side 1 = s (C[:M, :G] (+)= A . X[r0:r1], A's k = cell - r0, >= ceil((r1-r0)/64) * 64 deep)
extern "C" hipError_t cnmf_gemm_tiles(const unsigned short* A, long long lda, long long a_plane,
                                      int a_rows, int a_k, const unsigned* ent,
                                      const unsigned short* v1, const unsigned short* v2,
                                      const long long* tile_ptr, long long nnz, int n_cells,
                                      int n_genes, float* C, long long ldc, int c_cols,
                                      const float* col_scale, int M, int side, int r0, int r1,
                                      int pa, int pb, int accumulate, const int* gate,
                                      hipStream_t stream) {
  if (M <= 0 || r1 <= r0) return hipSuccess;
  if (pa < 2 || pa > 3 || pb < 1 || pb > 3 || side < 0 || side > 1 || r0 < 0 || r1 > n_cells ||
      n_genes < 1 || lda % 8 || a_plane % 8 || a_rows < 1 || nnz < 0 || !ent || !tile_ptr ||
      (pb >= 2 && !v1) || (pb >= 3 && !v2))
    return hipErrorInvalidValue;
  cnmf::TileGemmParams p;
  p.A = A; p.lda = lda; p.a_plane = a_plane; p.a_rows = a_rows;
  p.ent = ent; p.v1 = v1; p.v2 = v2; p.tile_ptr = tile_ptr; p.nnz = nnz;
  p.ntr = (n_cells + 63) / 64;
  p.ntg = (n_genes + 63) / 64;
  p.C = C; p.ldc = ldc; p.col_scale = col_scale;
  p.M = M; p.r0 = r0; p.r1 = r1; p.accumulate = accumulate; p.gate = gate;
  p.tiles_m = (M + 127) / 128;
  if (side == 0) {
    p.N = r1 - r0;
    p.nk = p.ntg;
    p.tiles_n = (r1 - 1) / 64 - r0 / 64 + 1;
  } else {
    p.N = n_genes;
    p.nk = (r1 - r0 + 63) / 64;
    p.tiles_n = p.ntg;
  }
  // A is read 64 k per step, C written up to column N
  if ((long long)p.nk * 64 > a_k || c_cols < p.N || ldc < p.N) return hipErrorInvalidValue;
  return cnmf::launch_tiles_planes(pa, pb, side, p, stream);
}
