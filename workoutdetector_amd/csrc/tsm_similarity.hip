// Temporal self-similarity: the cosine-distance matrix of unit rows (utils/common.py:118-143, plot_sim:
// pairwise_distances(feats, metric='cosine') -- "row-wise softmax. Repnet did this").
#include "tsm_device.h"

#include <cmath>

namespace tsm {

// ---------------------------------------------------------------------------------------------
// cosine_dist_kernel: D[i][j] = clamp(1 - <unit_i, unit_j>, 0, 2), D[i][i] = 0 (scikit-learn's cosine_distances with X is Y)
// for the band i in [row0, row1), j in [0, row1), and the mirror D[j][i] from the SAME computed value.
//
// Work: the band's elements with j <= i (everything else of the L-shaped region is their mirror: j > i with i in the band puts
// j in the band too).  They are cut into 64 x 64 tiles on the ABSOLUTE grid, tile (ti, tj) with tj <= ti and ti from
// row0 / 64 to (row1 - 1) / 64, numbered row by row; a workgroup of four waves (2 x 2, one 32 x 32 MFMA tile each) walks
// the numbers blockIdx.x, + gridDim.x, ... (64-bit: n_total is not limited by the grid).  Per 32 channels both panels go
// global -> registers -> LDS (16-byte loads, rows >= row1 and channels >= c read nothing and stage zeros), the next
// step's loads in flight under this step's 16 MFMAs.
//
// Arithmetic: v_mfma_f32_32x32x2_f32 (operand order: tsm_igemm.hip), an fp32 fma chain.  The instruction sums k = (lane half
// 0's, lane half 1's), so an LDS row holds its 32 channels de-interleaved -- [k even x16 | k odd x16] -- and half h reads
// 16 h + 4 g ..: step (g, e) multiplies channels 8 g + 2 e and 8 g + 2 e + 1.  Every element is ONE chain over k = 0 .. c - 1
// in ascending order (zero padding behind c adds +0), whichever band, tile, wave or launch computes it; there is no split-K and
// the operands are never swapped -- the upper triangle is written from the lower one's registers.
//
// Epilogue: D[i][j] straight from the accumulators (a lane half writes 32 consecutive floats); the mirror through a
// wave-private 32 x 33 LDS patch so that D[j][i] is written along i as well.  Masks: row0 <= i < row1, j <= i; the
// diagonal is stored as 0 once.  The kernel reads unit rows [0, row1) only and writes exactly that region.
// ---------------------------------------------------------------------------------------------
constexpr int kSimTile = 64;

__global__ void __launch_bounds__(256) cosine_dist_kernel(const float *__restrict__ unit, float *__restrict__ dist,
                                                          int n_total, int c, int row0, int row1, long long n_tiles,
                                                          long long tile_base) {
  __shared__ __attribute__((aligned(16))) float smem[2 * kSimTile * kLds];   // A panel | B panel; the epilogue's patches
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int half = lane >> 5, l31 = lane & 31;
  const int lrow = tid >> 3, lk = (tid & 7) * 4;   // loader: rows lrow and lrow + 32 of a panel, channels lk .. lk + 3 of the step
  const int nk = (c + kBK - 1) / kBK;

  for (long long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
    // tile number -> (ti, tj): row ti holds ti + 1 tiles, tile_base = those of the rows before row0's
    const long long g = t + tile_base;
    long long ti = (long long)((sqrt(8.0 * (double)g + 1.0) - 1.0) * 0.5);
    while (ti * (ti + 1) / 2 > g) --ti;
    while ((ti + 1) * (ti + 2) / 2 <= g) ++ti;
    const long long tj = g - ti * (ti + 1) / 2;
    const long long i0 = ti * kSimTile, j0 = tj * kSimTile;

    const float *src[4];   // A rows lrow, lrow + 32; B rows lrow, lrow + 32 (null: the row is outside [0, row1))
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long r = (q < 2 ? i0 : j0) + lrow + 32 * (q & 1);
      src[q] = r < row1 ? unit + r * (long long)c + lk : nullptr;
    }
    f32x4 regs[4];
    auto fetch = [&](int kt) {
      const bool in_k = kt * kBK + lk < c;
#pragma unroll
      for (int q = 0; q < 4; ++q)
        regs[q] = (src[q] && in_k) ? *reinterpret_cast<const f32x4 *>(src[q] + kt * kBK) : f32x4{0.f, 0.f, 0.f, 0.f};
    };
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    fetch(0);
    for (int kt = 0; kt < nk; ++kt) {
      __syncthreads();   // the previous step's fragments (and the previous tile's patches) have been read
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float *row = smem + ((q >> 1) * kSimTile + lrow + 32 * (q & 1)) * kLds + (lk >> 1);
        *reinterpret_cast<f32x2 *>(row) = f32x2{regs[q][0], regs[q][2]};        // even channels
        *reinterpret_cast<f32x2 *>(row + 16) = f32x2{regs[q][1], regs[q][3]};   // odd channels
      }
      __syncthreads();
      if (kt + 1 < nk) fetch(kt + 1);
      const float *As = smem + (wm * 32 + l31) * kLds + half * 16;
      const float *Bs = smem + (kSimTile + wn * 32 + l31) * kLds + half * 16;
#pragma unroll
      for (int g4 = 0; g4 < 4; ++g4) {
        const f32x4 a = *reinterpret_cast<const f32x4 *>(As + g4 * 4);
        const f32x4 b = *reinterpret_cast<const f32x4 *>(Bs + g4 * 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[e], b[e], acc, 0, 0, 0);
      }
    }
    __syncthreads();   // every wave is done with the panels: the patches overlay them

    const long long wi0 = i0 + wm * 32, wj0 = j0 + wn * 32;
    const bool active = wj0 <= wi0 + 31 && wi0 < row1 && wi0 + 31 >= row0;   // (wave-uniform: some of this wave's tile is in the region)
    float *patch = smem + wave * (32 * 33);
    if (active) {
      const long long j = wj0 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int il = (r & 3) + 8 * (r >> 2) + 4 * half;
        const long long i = wi0 + il;
        const float d = fminf(fmaxf(1.f - acc[r], 0.f), 2.f);
        patch[l31 * 33 + il] = d;
        if (i >= row0 && i < row1 && j <= i) dist[i * (long long)n_total + j] = i == j ? 0.f : d;
      }
    }
    __syncthreads();
    if (active) {
      const long long i = wi0 + l31;
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int jl = 2 * r + half;
        const long long jj = wj0 + jl;
        const float d = patch[jl * 33 + l31];
        if (i >= row0 && i < row1 && jj < i) dist[jj * (long long)n_total + i] = d;
      }
    }
  }
}

hipError_t launch_cosine_distances(const float *unit, int n_total, int c, int row0, int row1, float *dist, hipStream_t s) {
  if (!unit || !dist || row0 < 0 || row0 >= row1 || row1 > n_total || c <= 0 || c % 8 != 0) return hipErrorInvalidValue;
  const long long t0 = row0 / kSimTile, t1 = (row1 - 1) / kSimTile;
  const long long tile_base = t0 * (t0 + 1) / 2;
  const long long n_tiles = (t1 + 1) * (t1 + 2) / 2 - tile_base;
  const long long cap = 1 << 20;
  TSM_KLAUNCH(cosine_dist_kernel, dim3((unsigned)(n_tiles < cap ? n_tiles : cap)), dim3(256), 0, s, unit, dist, n_total, c, row0,
              row1, n_tiles, tile_base);
  return hipGetLastError();
}

}  // namespace tsm
