// Transposed tile CSRs of a row chunk of a CSR matrix, on the device (csr storage of the
// data matrix, models.nmf_base.SparseCSRX): for the chunk's c rows (cells) split into tiles
// of tl rows, the CSR of every tile's transpose -- G rows (genes), columns = the cell's
// index inside the tile, ascending within a gene -- which is what the spectra side of the
// sparse KL kernel (sparse_kl.hip, side 1) streams.  All tiles of the chunk share one
// col / val allocation (a tile's entries are contiguous in the source, so tile t starts at
// rowptr[t tl] - rowptr[0]) and carry absolute row pointers, (T, G + 1).
//
// Four launches, every tile in each:
//   count    one wave per source row: cnt[t][g] += 1 (integer atomics: order-free)
//   scan     one workgroup per tile: exclusive scan of cnt over the genes -> rowptrT, and
//            the same offsets back into cnt as the scatter's cursors
//   scatter  one wave per source row: (cell, value) to tmp[cursor[t][g]++] -- the order
//            inside a gene segment is whatever the atomics gave
//   place    a workgroup per (tile, gene) segment: the cells of a segment are unique and
//            < tl <= 8192, so a presence bitmap of 256 words in LDS ranks them -- rank =
//            set bits below the cell -- and every entry goes to segment start + rank.
// The result does not depend on the order of any atomic: two builds are identical.  No
// float atomics.  Indices are guarded (a column outside [0, G), entries outside [lo, hi))
// so that a malformed input cannot make the kernels write outside their arrays; such an
// input is rejected on the host before it gets here (SparseCSRX._validate).
#include <hip/hip_runtime.h>

namespace cnmf {

constexpr int kCtThreads = 256;
constexpr int kCtWaves = kCtThreads / 64;
constexpr int kCtMaxTile = 8192;                 // cells per tile: 256 bitmap words
constexpr int kCtWords = kCtMaxTile / 32;
constexpr int kCtMaxGrid = 1 << 20;              // place: workgroups (each loops over segments)

// entries [e0, e1) of source row i, clamped to the chunk's own range [lo, hi)
__device__ __forceinline__ void ct_row_range(const int* __restrict__ rowptr, int i, int lo,
                                             int hi, int& e0, int& e1) {
  e0 = max(rowptr[i], lo);
  e1 = min(rowptr[i + 1], hi);
}

template <bool kScatter>
__global__ __launch_bounds__(kCtThreads) void ct_rows_kernel(
    const int* __restrict__ rowptr, const int* __restrict__ col, const float* __restrict__ val,
    int c, int G, int tl, int lo, int hi, int* __restrict__ cnt, int2* __restrict__ tmp) {
  const int i = blockIdx.x * kCtWaves + (threadIdx.x >> 6);
  if (i >= c) return;
  const int lane = threadIdx.x & 63;
  const int t = i / tl;
  const int cell = i - t * tl;
  int e0, e1;
  ct_row_range(rowptr, i, lo, hi, e0, e1);
  int* __restrict__ row = cnt + (long long)t * G;
  for (int e = e0 + lane; e < e1; e += 64) {
    const int g = col[e];
    if ((unsigned)g >= (unsigned)G) continue;
    if (!kScatter) {
      atomicAdd(&row[g], 1);
    } else {
      const int pos = atomicAdd(&row[g], 1);
      if ((unsigned)pos < (unsigned)(hi - lo)) tmp[pos] = make_int2(cell, __float_as_int(val[e]));
    }
  }
}

// inclusive scan of v over the workgroup; returns this thread's inclusive sum, total in tot
__device__ __forceinline__ int ct_block_scan(int v, int* wsum, int& tot) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int s = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const int u = __shfl_up(s, d, 64);
    if (lane >= d) s += u;
  }
  if (lane == 63) wsum[w] = s;
  __syncthreads();
  int off = 0;
  tot = 0;
#pragma unroll
  for (int j = 0; j < kCtWaves; ++j) {
    const int x = wsum[j];
    if (j < w) off += x;
    tot += x;
  }
  __syncthreads();
  return s + off;
}

__global__ __launch_bounds__(kCtThreads) void ct_scan_kernel(
    const int* __restrict__ rowptr, int c, int G, int tl, int lo, int hi, int* __restrict__ cnt,
    int* __restrict__ rowptrT) {
  __shared__ int wsum[kCtWaves];
  const int t = blockIdx.x;
  int* __restrict__ row = cnt + (long long)t * G;
  int* __restrict__ out = rowptrT + (long long)t * (G + 1);
  int carry = min(max(rowptr[min(t * tl, c)], lo), hi) - lo;      // the tile's first entry
  for (int g0 = 0; g0 < G; g0 += kCtThreads) {
    const int g = g0 + threadIdx.x;
    const int v = g < G ? row[g] : 0;
    int tot;
    const int inc = ct_block_scan(v, wsum, tot);
    if (g < G) {
      out[g] = carry + inc - v;
      row[g] = carry + inc - v;
    }
    carry += tot;
  }
  if (threadIdx.x == 0) out[G] = carry;
}

__global__ __launch_bounds__(kCtThreads) void ct_place_kernel(
    const int* __restrict__ rowptrT, int G, int n_seg, int n_ent,
    const int2* __restrict__ tmp,
    int* __restrict__ colT, float* __restrict__ valT) {
  __shared__ unsigned bits[kCtWords];
  __shared__ int pre[kCtWords];
  __shared__ int wsum[kCtWaves];
  static_assert(kCtWords == kCtThreads, "one bitmap word per thread");
  for (int seg = blockIdx.x; seg < n_seg; seg += gridDim.x) {
    const int t = seg / G, g = seg - t * G;
    const int* __restrict__ rp = rowptrT + (long long)t * (G + 1) + g;
    const int s0 = max(rp[0], 0);
    const int s1 = min(rp[1], n_ent);
    const int n = s1 - s0;
    if (n <= 0) continue;                  // (uniform over the workgroup)
    if (n == 1) {
      if (threadIdx.x == 0) {
        const int2 e = tmp[s0];
        colT[s0] = e.x;
        valT[s0] = __int_as_float(e.y);
      }
      continue;
    }
    bits[threadIdx.x] = 0u;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kCtThreads) {
      const unsigned cell = (unsigned)tmp[s0 + j].x & (kCtMaxTile - 1);
      atomicOr(&bits[cell >> 5], 1u << (cell & 31));
    }
    __syncthreads();
    const int v = __popc(bits[threadIdx.x]);
    int tot;
    const int inc = ct_block_scan(v, wsum, tot);
    pre[threadIdx.x] = inc - v;
    __syncthreads();
    for (int j = threadIdx.x; j < n; j += kCtThreads) {
      const int2 e = tmp[s0 + j];
      const unsigned cell = (unsigned)e.x & (kCtMaxTile - 1);
      const int rank = pre[cell >> 5] + __popc(bits[cell >> 5] & ((1u << (cell & 31)) - 1u));
      if (rank < n) {
        colT[s0 + rank] = e.x;
        valT[s0 + rank] = __int_as_float(e.y);
      }
    }
    __syncthreads();                       // bits / pre are reused by the next segment
  }
}

// ---- the transpose of the whole matrix: the tile transposes merged per gene.  A gene's
// row is its tile segments one after the other (tiles ascend in cell index, a segment
// ascends inside its tile), so the entries of a row are ordered by cell.  Three launches:
//   prefix  one thread per gene: pre[t][g] = entries of gene g in the tiles before t, tot[g]
//   scan    one workgroup: exclusive scan of tot over the genes -> the global row pointers
//   merge   one wave per (tile, gene) segment: copied to rowptr[g] + pre[t][g], the cell
//           index made global.  No atomics at all.
__global__ __launch_bounds__(kCtThreads) void ct_gene_prefix_kernel(
    const int* __restrict__ rowptrT, int T, int G, int* __restrict__ pre,
    int* __restrict__ tot) {
  const int g = blockIdx.x * kCtThreads + threadIdx.x;
  if (g >= G) return;
  int run = 0;
  for (int t = 0; t < T; ++t) {
    const int* __restrict__ rp = rowptrT + (long long)t * (G + 1) + g;
    pre[(long long)t * G + g] = run;
    run += max(rp[1] - rp[0], 0);
  }
  tot[g] = run;
}

__global__ __launch_bounds__(kCtThreads) void ct_total_scan_kernel(
    const int* __restrict__ tot, int G, int* __restrict__ out) {
  __shared__ int wsum[kCtWaves];
  int carry = 0;
  for (int g0 = 0; g0 < G; g0 += kCtThreads) {
    const int g = g0 + threadIdx.x;
    const int v = g < G ? tot[g] : 0;
    int sum;
    const int inc = ct_block_scan(v, wsum, sum);
    if (g < G) out[g] = carry + inc - v;
    carry += sum;
  }
  if (threadIdx.x == 0) out[G] = carry;
}

__global__ __launch_bounds__(kCtThreads) void ct_merge_kernel(
    const int* __restrict__ rowptrT, int G, int tl, long long n_seg, int n_ent,
    const int* __restrict__ pre, const int* __restrict__ rowptrG,
    const int* __restrict__ colT, const float* __restrict__ valT, int* __restrict__ colG,
    float* __restrict__ valG) {
  const int lane = threadIdx.x & 63;
  const long long step = (long long)gridDim.x * kCtWaves;
  for (long long seg = (long long)blockIdx.x * kCtWaves + (threadIdx.x >> 6); seg < n_seg;
       seg += step) {
    const int t = (int)(seg / G), g = (int)(seg - (long long)t * G);
    const int* __restrict__ rp = rowptrT + (long long)t * (G + 1) + g;
    const int s0 = max(rp[0], 0);
    const int s1 = min(rp[1], n_ent);
    const int d0 = rowptrG[g] + pre[seg];
    const int cell0 = t * tl;
    for (int j = lane; j < s1 - s0; j += 64) {
      const int d = d0 + j;
      if ((unsigned)d < (unsigned)n_ent) {
        colG[d] = colT[s0 + j] + cell0;
        valG[d] = valT[s0 + j];
      }
    }
  }
}

}  // namespace cnmf

extern "C" int cnmf_csr_transpose_max_tile() { return cnmf::kCtMaxTile; }

// rowptr: the chunk's c + 1 absolute offsets into col / val, all within [lo, hi) = the
// chunk's entries (lo = rowptr[0], hi = rowptr[c], read by the caller).  cnt: (T, G) int
// workspace; tmp: hi - lo entries; rowptrT (T, G + 1); colT / valT: hi - lo entries,
// T = ceil(c / tl).
extern "C" hipError_t cnmf_csr_transpose_tiles(const int* rowptr, const int* col,
                                               const float* val, int c, int G, int tl, int lo,
                                               int hi, int* cnt, void* tmp, int* rowptrT,
                                               int* colT, float* valT, hipStream_t stream) {
  using namespace cnmf;
  if (c < 0 || G < 0 || tl < 1 || tl > kCtMaxTile || lo < 0 || hi < lo)
    return hipErrorInvalidValue;
  if (c == 0 || G == 0) return hipSuccess;
  const long long T = ((long long)c + tl - 1) / tl;
  if (T * G > 0x7fffffffLL) return hipErrorInvalidValue;
  hipError_t err = hipMemsetAsync(cnt, 0, sizeof(int) * (size_t)(T * G), stream);
  if (err != hipSuccess) return err;
  const dim3 rows((c + kCtWaves - 1) / kCtWaves), blk(kCtThreads);
  int2* tmp2 = static_cast<int2*>(tmp);
  hipLaunchKernelGGL(ct_rows_kernel<false>, rows, blk, 0, stream, rowptr, col, val, c, G, tl, lo,
                     hi, cnt, tmp2);
  hipLaunchKernelGGL(ct_scan_kernel, dim3((unsigned)T), blk, 0, stream, rowptr, c, G, tl, lo, hi,
                     cnt, rowptrT);
  if (hi > lo) {
    hipLaunchKernelGGL(ct_rows_kernel<true>, rows, blk, 0, stream, rowptr, col, val, c, G, tl,
                       lo, hi, cnt, tmp2);
    const long long n_seg = T * G;
    hipLaunchKernelGGL(ct_place_kernel, dim3((unsigned)(n_seg < kCtMaxGrid ? n_seg : kCtMaxGrid)),
                       blk, 0, stream, rowptrT, G, (int)n_seg, hi - lo, tmp2, colT, valT);
  }
  return hipGetLastError();
}

// The transpose of the whole matrix from its tile transposes (cnmf_csr_transpose_tiles with
// the same T, G, tl; n_ent entries): rowptrG (G + 1, from 0), colG / valG (n_ent), the
// entries of a row ordered by cell.  pre: (T, G) int workspace, tot: (G).
extern "C" hipError_t cnmf_csr_transpose_merge(const int* rowptrT, const int* colT,
                                               const float* valT, int T, int G, int tl,
                                               int n_ent, int* pre, int* tot, int* rowptrG,
                                               int* colG, float* valG, hipStream_t stream) {
  using namespace cnmf;
  if (T < 0 || G < 0 || tl < 1 || tl > kCtMaxTile || n_ent < 0 ||
      (long long)T * tl > 0x7fffffffLL)
    return hipErrorInvalidValue;
  if (G == 0) return hipSuccess;
  const dim3 blk(kCtThreads);
  hipLaunchKernelGGL(ct_gene_prefix_kernel, dim3((G + kCtThreads - 1) / kCtThreads), blk, 0,
                     stream, rowptrT, T, G, pre, tot);
  hipLaunchKernelGGL(ct_total_scan_kernel, dim3(1), blk, 0, stream, tot, G, rowptrG);
  const long long n_seg = (long long)T * G;
  if (n_seg > 0 && n_ent > 0) {
    const long long wgs = (n_seg + kCtWaves - 1) / kCtWaves;
    hipLaunchKernelGGL(ct_merge_kernel, dim3((unsigned)(wgs < kCtMaxGrid ? wgs : kCtMaxGrid)),
                       blk, 0, stream, rowptrT, G, tl, n_seg, n_ent, pre, rowptrG, colT, valT,
                       colG, valG);
  }
  return hipGetLastError();
}
