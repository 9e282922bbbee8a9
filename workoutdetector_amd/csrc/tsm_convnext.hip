// The non-GEMM part of a ConvNeXt-Base image model (tsm_set_convnext; timm 0.5.4 convnext_base), fp32, NHWC:
//   dwconv7_ln_kernel<C>   depthwise 7x7 (padding 3, bias) + the LayerNorm behind it, one launch per block
//   ln_kernel<C, S2D>      LayerNorm per pixel: the stem's and the head's (S2D = false), and a downsample's, which writes the 2x2
//                          space-to-depth rows its strided conv then reads as a 1x1 GEMM (S2D = true)
//   stem_pack4_kernel      the packed input [n, H, W, 4] -> the stem's 4x4 patches [n, H / 4, W / 4, 64]
//   gelu_kernel            exact GELU, in place, between fc1 and fc2
// Every matrix product of the network (stem, downsamples, fc1, fc2) runs on conv_igemm as a 1x1 conv.
//
// One lane mapping for everything that normalises: a pixel's C channels are spread over C / 4 consecutive lanes, four consecutive
// channels (16 bytes) per lane -- 32 lanes (half a wave) at C = 128, one wave at 256, two at 512, four at 1024.  Global accesses
// are then 16 bytes per lane and contiguous over the lanes of a pixel, a depthwise tap's weights [49][C] are read the same way,
// and the conv itself needs no exchange between lanes at all: a lane keeps its four channels for every tap, so the 7x7 window's
// reuse happens in its own registers and LDS carries nothing but the cross-wave partial sums of the LayerNorm (C >= 512).
//
// LayerNorm (biased variance, eps 1e-6, affine), two passes, each in an order that depends on C alone:
//   a lane adds its four values ((v0 + v1) + v2) + v3; the lanes of a wave combine in a butterfly (xor 1, 2, 4, 8, 16 and, for
//   C >= 256, 32: every lane of the pixel ends with the same bits, since each step adds the same two numbers on both sides); for
//   C >= 512 the pixel's waves leave their sums in LDS and every lane adds them in ascending wave order.
//   mean = sum / C; then the same reduction over (v - mean)^2; y = (v - mean) / sqrt(var + eps) * weight + bias.
// Nothing depends on the number of frames, the grid or on which frames share the launch; no atomics.
#include "tsm_device.h"
#include "tsm_host_util.h"   // kCnx*, cnx_s2d_k, cnx_stem_k, cnx_dw_tiles: the sizes tests/convnext_host.cpp checks

#include <cmath>

namespace tsm {

namespace {

constexpr int kCnxThreads = 256;

// Sums v[i] over the C / 4 lanes of the calling lane's pixel group, for NP independent values at once (see the file comment).
// red: LDS [4][NP], one row per wave of the workgroup, used when a pixel spans more than one wave; every thread of the
// workgroup must call (the cross-wave step holds a barrier).
template <int C, int NP>
__device__ __forceinline__ void group_sum(float (&v)[NP], float (*red)[NP]) {
  constexpr int L = C / 4, WL = L < 64 ? L : 64;
#pragma unroll
  for (int off = 1; off < WL; off <<= 1) {
#pragma unroll
    for (int i = 0; i < NP; ++i) v[i] += __shfl_xor(v[i], off, 64);
  }
  if constexpr (L > 64) {
    constexpr int WAVES = L / 64;
    const int wave = threadIdx.x >> 6, first = wave / WAVES * WAVES;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int i = 0; i < NP; ++i) red[wave][i] = v[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      float s = red[first][i];
#pragma unroll
      for (int k = 1; k < WAVES; ++k) s += red[first + k][i];
      v[i] = s;
    }
  }
}

__device__ __forceinline__ float sum4(const f32x4 &a) { return ((a[0] + a[1]) + a[2]) + a[3]; }

// The LayerNorm of NP pixels held as one channel quad per lane: v[i] -> its normalised, scaled and shifted value.
template <int C, int NP>
__device__ __forceinline__ void layer_norm(f32x4 (&v)[NP], const f32x4 &weight, const f32x4 &bias, float (*red_a)[NP], float (*red_b)[NP]) {
  float s[NP];
#pragma unroll
  for (int i = 0; i < NP; ++i) s[i] = sum4(v[i]);
  group_sum<C, NP>(s, red_a);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    v[i] -= s[i] / (float)C;
    s[i] = sum4(v[i] * v[i]);
  }
  group_sum<C, NP>(s, red_b);
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    const float rstd = 1.0f / sqrtf(s[i] / (float)C + tsm_host::kCnxLnEps);
    v[i] = v[i] * rstd * weight + bias;
  }
}

}  // namespace

// ---------------------------------------------------------------------------------------------
// dwconv7_ln_kernel<C>: y[n, oy, ox, :] = LayerNorm_c( b[c] + sum_{ky, kx} w[ky][kx][c] x[n, oy + ky - 3, ox + kx - 3, c] ).
// x, y [n, H, W, C]; w [49][C] (tsm_host::cnx_pack_dw); the un-normalised conv output exists in registers only.
//
// A lane group (C / 4 lanes) owns one tile of TS x TS output pixels, TS = tsm_host::cnx_dw_tile(C): 4, at C = 1024 2; a workgroup of 256 threads holds 1024 / C of them (8, 4, 2, 1), tiles numbered frame-major over the launch.
// A lane keeps the TS x TS x 4 accumulators of its channel quad and walks the tile's TS + 6 input rows top down: a row is TS + 6
// quads (16-byte loads), and feeds the up to TS output rows it lies under, each with the 7 taps of its ky -- so every output
// element is ONE fmaf chain that starts from the bias and runs ky-major, kx inside, as the operator is written.  A row outside
// the frame is skipped as a whole and a column outside it is not loaded: its taps multiply a zero that never came from memory,
// which adds +-0 to a chain.  At TS = 4 each input quad is loaded once per tile (6.25 loads per output against 49 taps) and the
// weights are re-read per (row, output row) pair, 196 quads per tile that stay in the L1 / L2 (25 - 200 KB per layer).  The
// last stage's maps are small (7 x 7 at 224 x 224: 4 x 4 tiles compute 64 pixels for 49 and a 32-frame launch is 128 workgroups,
// half the CUs): it takes 2 x 2 tiles -- four times the lanes, 16 loads per output, all from the L2; measured 18 against 23 us.
// Stage 2 (14 x 14) was measured both ways too and stays at 4 x 4 (27 against 29 us).  Tiles at the right / bottom edge compute pixels past the frame from zeros and do not store them; the
// group behind the launch's last tile repeats that tile and stores nothing (every lane reaches the LayerNorm's barrier).
// Budget at TS = 4: 64 accumulators + 40 row registers + the taps in flight and the addressing, no scratch, 1 KB of LDS.
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(kCnxThreads) dwconv7_ln_kernel(const float *__restrict__ x, const float *__restrict__ w,
                                                                 const float *__restrict__ b, const float *__restrict__ ln_w,
                                                                 const float *__restrict__ ln_b, float *__restrict__ y, int H, int W,
                                                                 int tiles_y, int tiles_x, int n_tiles) {
  constexpr int L = C / 4, G = kCnxThreads / L, TS = tsm_host::cnx_dw_tile(C);
  static_assert(C == 128 || C == 256 || C == 512 || C == 1024, "ConvNeXt-Base widths");
  __shared__ float red_a[4][TS * TS], red_b[4][TS * TS];
  const int c = (threadIdx.x % L) * 4;
  int tile = blockIdx.x * G + threadIdx.x / L;
  const bool live = tile < n_tiles;
  if (!live) tile = n_tiles - 1;
  const int tx = tile % tiles_x, ty = tile / tiles_x % tiles_y;
  const int64_t f = tile / tiles_x / tiles_y;
  const int y0 = ty * TS, x0 = tx * TS;
  const float *xf = x + f * H * W * C + c;

  const f32x4 bias = *reinterpret_cast<const f32x4 *>(b + c);
  f32x4 acc[TS * TS];
#pragma unroll
  for (int i = 0; i < TS * TS; ++i) acc[i] = bias;
  static_for<TS + 6>([&](auto R) {
    constexpr int r = R;
    const int iy = y0 - 3 + r;
    if (iy >= 0 && iy < H) {
      f32x4 in[TS + 6];
      const float *row = xf + (int64_t)iy * W * C;
#pragma unroll
      for (int j = 0; j < TS + 6; ++j) {
        const int ix = x0 - 3 + j;
        in[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ix >= 0 && ix < W) in[j] = *reinterpret_cast<const f32x4 *>(row + (int64_t)ix * C);
      }
      static_for<TS>([&](auto OY) {
        constexpr int oy = OY, ky = r - oy;
        if constexpr (ky >= 0 && ky < 7) {
#pragma unroll
          for (int kx = 0; kx < 7; ++kx) {
            const f32x4 wv = *reinterpret_cast<const f32x4 *>(w + (ky * 7 + kx) * C + c);
#pragma unroll
            for (int ox = 0; ox < TS; ++ox) {
#pragma unroll
              for (int e = 0; e < 4; ++e) acc[oy * TS + ox][e] = fmaf(wv[e], in[ox + kx][e], acc[oy * TS + ox][e]);
            }
          }
        }
      });
    }
  });

  layer_norm<C, TS * TS>(acc, *reinterpret_cast<const f32x4 *>(ln_w + c), *reinterpret_cast<const f32x4 *>(ln_b + c), red_a, red_b);
  if (!live) return;
  float *yf = y + f * H * W * C + c;
#pragma unroll
  for (int oy = 0; oy < TS; ++oy) {
#pragma unroll
    for (int ox = 0; ox < TS; ++ox)
      if (y0 + oy < H && x0 + ox < W) *reinterpret_cast<f32x4 *>(yf + ((int64_t)(y0 + oy) * W + x0 + ox) * C) = acc[oy * TS + ox];
  }
}

hipError_t launch_dwconv7_ln(const float *x, const float *w, const float *b, const float *ln_w, const float *ln_b, float *y, int n,
                             int h, int wi, int c, hipStream_t s) {
  if (c != 128 && c != 256 && c != 512 && c != 1024) return hipErrorInvalidValue;
  const int ts = tsm_host::cnx_dw_tile(c);
  const int64_t tiles = tsm_host::cnx_dw_tiles(n, h, wi, ts);
  if (!x || !w || !b || !ln_w || !ln_b || !y || tiles <= 0) return hipErrorInvalidValue;
  const int ty = tsm_host::cnx_tiles_along(h, ts), tx = tsm_host::cnx_tiles_along(wi, ts);
#define TSM_DWLN(CH)                                                                                                             \
  TSM_KLAUNCH(dwconv7_ln_kernel<CH>, dim3((unsigned)((tiles + kCnxThreads / (CH / 4) - 1) / (kCnxThreads / (CH / 4)))), dim3(kCnxThreads), \
              0, s, x, w, b, ln_w, ln_b, y, h, wi, ty, tx, (int)tiles)
  if (c == 128) TSM_DWLN(128);
  else if (c == 256) TSM_DWLN(256);
  else if (c == 512) TSM_DWLN(512);
  else TSM_DWLN(1024);
#undef TSM_DWLN
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// ln_kernel<C, S2D>: LayerNorm of one pixel per lane group, 1024 / C pixels per workgroup.
// S2D = false: rows [n_rows][C] in, the same out (the stem's output; the head's pooled rows).
// S2D = true: x is [n, H, W, C] and the rows are the pixels (y, x) with y < 2 (H / 2), x < 2 (W / 2), frame-major; pixel (y, x) goes
// to the channels cnx_s2d_k(y, x, 0, C) .. + C - 1 of row (y / 2, x / 2) of out [n, H / 2, W / 2, 4 C]: the K order of a packed 2x2
// weight matrix.  A last odd row / column of the frame is neither read nor written (the strided conv drops it).
// ---------------------------------------------------------------------------------------------
template <int C, bool S2D>
__global__ void __launch_bounds__(kCnxThreads) ln_kernel(const float *__restrict__ x, const float *__restrict__ ln_w,
                                                         const float *__restrict__ ln_b, float *__restrict__ y, int64_t n_rows, int H,
                                                         int W) {
  constexpr int L = C / 4, G = kCnxThreads / L;
  __shared__ float red_a[4][1], red_b[4][1];
  const int c = (threadIdx.x % L) * 4;
  int64_t row = (int64_t)blockIdx.x * G + threadIdx.x / L;
  const bool live = row < n_rows;
  if (!live) row = n_rows - 1;
  int64_t src = row, dst = row * C;
  if constexpr (S2D) {
    const int ho = H / 2, wo = W / 2;
    const int px = (int)(row % (2 * wo)), py = (int)(row / (2 * wo) % (2 * ho));
    const int64_t f = row / (2 * wo) / (2 * ho);
    src = (f * H + py) * W + px;
    dst = ((f * ho + py / 2) * wo + px / 2) * (4 * (int64_t)C) + tsm_host::cnx_s2d_k(py, px, 0, C);
  }
  f32x4 v[1] = {*reinterpret_cast<const f32x4 *>(x + src * C + c)};
  layer_norm<C, 1>(v, *reinterpret_cast<const f32x4 *>(ln_w + c), *reinterpret_cast<const f32x4 *>(ln_b + c), red_a, red_b);
  if (live) *reinterpret_cast<f32x4 *>(y + dst + c) = v[0];
}

template <bool S2D>
static hipError_t launch_ln(const float *x, const float *ln_w, const float *ln_b, float *y, int64_t rows, int h, int w, int c, hipStream_t s) {
  if (!x || !ln_w || !ln_b || !y || rows <= 0 || c < 128 || c > 1024 || (c & (c - 1))) return hipErrorInvalidValue;
  const int64_t blocks = (rows + kCnxThreads / (c / 4) - 1) / (kCnxThreads / (c / 4));
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
#define TSM_LN(CH) TSM_KLAUNCH((ln_kernel<CH, S2D>), dim3((unsigned)blocks), dim3(kCnxThreads), 0, s, x, ln_w, ln_b, y, rows, h, w)
  if (c == 128) TSM_LN(128);
  else if (c == 256) TSM_LN(256);
  else if (c == 512) TSM_LN(512);
  else TSM_LN(1024);
#undef TSM_LN
  return hipGetLastError();
}

hipError_t launch_layer_norm(const float *x, const float *ln_w, const float *ln_b, float *y, int64_t rows, int c, hipStream_t s) {
  return launch_ln<false>(x, ln_w, ln_b, y, rows, 0, 0, c, s);
}

hipError_t launch_layer_norm_s2d(const float *x, const float *ln_w, const float *ln_b, float *y, int n, int h, int w, int c, hipStream_t s) {
  const int ho = tsm_host::cnx_down_size(h), wo = tsm_host::cnx_down_size(w);
  if (n <= 0 || ho <= 0 || wo <= 0) return hipErrorInvalidValue;
  return launch_ln<true>(x, ln_w, ln_b, y, (int64_t)n * (2 * ho) * (2 * wo), h, w, c, s);
}

// ---------------------------------------------------------------------------------------------
// stem_pack4_kernel: the stem's 4x4 / stride-4 patches.  x [n, H, W, 4] (the engine's packed fp32 input: r, g, b, 0) ->
// y [n, H / 4, W / 4, 64], K = cnx_stem_k(ky, kx, c).  One thread per tap: a 16-byte copy, channel 3 written as zero whatever
// the input holds there (its weights are zero, but 0 * NaN is not).  The last H % 4 rows / W % 4 columns are not read.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) stem_pack4_kernel(const float *__restrict__ x, float *__restrict__ y, int64_t n_taps, int H, int W) {
  const int ho = H / 4, wo = W / 4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_taps; i += stride) {
    const int t = (int)(i & 15);
    int64_t pix = i >> 4;
    const int ox = (int)(pix % wo);
    pix /= wo;
    const int oy = (int)(pix % ho);
    const int64_t f = pix / ho;
    f32x4 v = *reinterpret_cast<const f32x4 *>(x + ((f * H + 4 * oy + (t >> 2)) * W + 4 * ox + (t & 3)) * 4);
    v[3] = 0.f;
    *reinterpret_cast<f32x4 *>(y + i * 4) = v;
  }
}

hipError_t launch_stem_pack4(const float *x, float *y, int n, int h, int w, hipStream_t s) {
  const int ho = tsm_host::cnx_stem_size(h), wo = tsm_host::cnx_stem_size(w);
  if (!x || !y || n <= 0 || ho <= 0 || wo <= 0) return hipErrorInvalidValue;
  const int64_t taps = (int64_t)n * ho * wo * 16;
  TSM_KLAUNCH(stem_pack4_kernel, dim3(grid_for(taps, 8192)), dim3(256), 0, s, x, y, taps, h, w);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gelu_kernel: x = 0.5 x (1 + erf(x / sqrt 2)) in place over n4 quads.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gelu_kernel(float *__restrict__ x, int64_t n4) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 v = *reinterpret_cast<const f32x4 *>(x + i * 4);
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = 0.5f * v[e] * (1.0f + erff(v[e] * 0.70710678118654752440f));
    *reinterpret_cast<f32x4 *>(x + i * 4) = v;
  }
}

hipError_t launch_gelu(float *x, int64_t n4, hipStream_t s) {
  if (!x || n4 <= 0) return hipErrorInvalidValue;
  TSM_KLAUNCH(gelu_kernel, dim3(grid_for(n4, 16384)), dim3(256), 0, s, x, n4);
  return hipGetLastError();
}

}  // namespace tsm
