// The non-GEMM part of a TDN-ResNet50 (tsm_set_tdn; include/tsm_hip.h holds the network's definition), fp32, NHWC:
//   tdn_front_kernel             the difference front end: the 15 input planes of a segment -> the centre frame as packed NHWC4 (what
//                                the fp32 stem reads in place) and conv1_5's patch rows [frames * H/4 * W/4][1024], K = (ky, kx, c)
//   tdn_front_pool_kernel        the same from a pool of transformed frames (TSM_LAYOUT_TDN_POOL): the planes found by a table or a window rule
//   tdn_fuse_kernel              x <- alpha x + beta up(d) in place, torch's 'nearest' upsample
//   mse_squeeze_kernel<R>        b = BN(W1 x): C = 16 R channels -> R, the only reader of conv1's output besides the excite kernel
//   mse_diff_kernel<R>           c = depthwise 3x3 of b (never stored), d+[t] = c[t + 1] - b[t], d-[t] = c[t - 1] - b[t] (zero at the
//                                clip's last / first frame) and their 2x2 average pools
//   mse_s2_kernel<R>             s2 = BN(K2 * pooled d), both directions, on the pooled map
//   mse_mix_kernel<R>            s4 = BN(K4 * d) and m = d / 3 + up(s2) / 3 + s4 / 3, both directions
//   mse_excite_shift_kernel<C>   e = BN(W3 m), y = (sigmoid(e+) - 1/2) / 2 + (sigmoid(e-) - 1/2) / 2, g = x + x y, and the learned 3-tap
//                                temporal conv o[t] = w0 g[t - 1] + w1 g[t] + w2 g[t + 1] behind it: g never reaches memory
// Everything between the squeeze and the excite lives in R-channel maps, 1 / 16 of conv1's width; the R -> R 3x3 convs are plain
// FMAs (under 1 % of a block's FLOPs).
//
// Every output element has ONE summation order, fixed by the layer alone: nothing depends on the number of frames, the grid or on
// which clips share a launch; no atomics.  Full-precision expf and division in the sigmoid.
#include "tsm_device.h"
#include "tsm_host_util.h"   // kTdn*, tdn_nearest, tdn_patch_k: the arithmetic tests/tdn_host.cpp checks

#include <cmath>

namespace tsm {

constexpr int kTdnThreads = 256;
constexpr int kPT = 2 * tsm_host::kTdnTile + 5;   // side of the pooled-difference tile a workgroup stages: 21

// ---------------------------------------------------------------------------------------------
// tdn_front_kernel.  x [n, 15, H, W] (planes f0.rgb .. f4.rgb), H and W multiples of 32.  One workgroup per frame and 8 x 8 tile
// of conv1_5 outputs.  Phase 1: the 21 x 21 x 12 tile of P = avgpool2x2(concat(f1 - f0, f2 - f1, f3 - f2, f4 - f3)) that those
// outputs read goes to LDS, zeros where it leaves the map (the conv's padding); a thread that owns one of the tile's inner
// 16 x 16 cells also writes its 2 x 2 centre-frame pixels (planes 6 .. 8) to in4 [n, H, W, 4] -- the inner cells of all tiles
// partition the frame.  Phase 2: the 64 patch rows, 1024 floats each: row ky of a patch is 84 contiguous floats of the LDS
// tile, the K tail from 588 on is zero.  P and the differences never reach memory.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTdnThreads) tdn_front_kernel(const float *__restrict__ x, float *__restrict__ in4,
                                                                float *__restrict__ patches, int H, int W) {
  using namespace tsm_host;
  __shared__ __attribute__((aligned(16))) float tile[kPT * kPT * kTdnDiffC];
  const int hp = H / 2, wp = W / 2, ho = H / 4, wo = W / 4;
  const int tiles_x = wo / kTdnTile;
  const int oy0 = (int)(blockIdx.x / tiles_x) * kTdnTile, ox0 = (int)(blockIdx.x % tiles_x) * kTdnTile;
  const int64_t f = blockIdx.y;
  const float *xf = x + f * kTdnPlanes * (int64_t)H * W;
  for (int idx = threadIdx.x; idx < kPT * kPT; idx += kTdnThreads) {
    const int ty = idx / kPT, tx = idx - ty * kPT;
    const int py = 2 * oy0 - 3 + ty, px = 2 * ox0 - 3 + tx;
    float p[kTdnDiffC];
#pragma unroll
    for (int c = 0; c < kTdnDiffC; ++c) p[c] = 0.f;
    if (py >= 0 && py < hp && px >= 0 && px < wp) {
      f32x2 v[kTdnPlanes][2];
#pragma unroll
      for (int pl = 0; pl < kTdnPlanes; ++pl)
#pragma unroll
        for (int r = 0; r < 2; ++r) v[pl][r] = *reinterpret_cast<const f32x2 *>(xf + ((int64_t)pl * H + 2 * py + r) * W + 2 * px);
#pragma unroll
      for (int c = 0; c < kTdnDiffC; ++c) {
        const f32x2 d0 = v[c + 3][0] - v[c][0], d1 = v[c + 3][1] - v[c][1];
        p[c] = ((d0[0] + d0[1]) + (d1[0] + d1[1])) * 0.25f;
      }
      if (ty >= 3 && ty < 3 + 2 * kTdnTile && tx >= 3 && tx < 3 + 2 * kTdnTile) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const f32x4 px4 = {v[6][r][q], v[7][r][q], v[8][r][q], 0.f};
            *reinterpret_cast<f32x4 *>(in4 + ((f * H + 2 * py + r) * W + 2 * px + q) * 4) = px4;
          }
      }
    }
#pragma unroll
    for (int c4 = 0; c4 < kTdnDiffC / 4; ++c4) {
      const f32x4 o = {p[4 * c4], p[4 * c4 + 1], p[4 * c4 + 2], p[4 * c4 + 3]};
      *reinterpret_cast<f32x4 *>(tile + idx * kTdnDiffC + 4 * c4) = o;
    }
  }
  __syncthreads();
  // a thread keeps its K quad for all 64 rows: one row (4 KB) per pass of the workgroup
  const int k = 4 * (int)threadIdx.x;
  const bool real = k < kTdnPatchReal;
  const int ky = k / (7 * kTdnDiffC), rem = k - ky * (7 * kTdnDiffC);
  for (int row = 0; row < kTdnTile * kTdnTile; ++row) {
    const int oyl = row / kTdnTile, oxl = row - oyl * kTdnTile;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (real) o = *reinterpret_cast<const f32x4 *>(tile + ((2 * oyl + ky) * kPT + 2 * oxl) * kTdnDiffC + rem);
    *reinterpret_cast<f32x4 *>(patches + ((f * ho + oy0 + oyl) * wo + ox0 + oxl) * kTdnPatchK + k) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// tdn_front_pool_kernel (TSM_LAYOUT_TDN_POOL): tdn_front_kernel with its 15 planes found in a pool of transformed frames
// [n_frames, 3, H, W]: plane pl of segment blockIdx.y is channel pl % 3 of pool frame frame_of(segment, pl / 3), from the table
// (mode 0: src.index [segments][5], an entry outside the pool stands for planes of 0.0f) or from the window rule (mode 1:
// tsm_host::tdn_window_frame).  The five frame numbers depend on blockIdx alone: they are fetched (scalar loads) or computed once
// per workgroup and live in scalar registers; a missing frame is a null pointer and a uniform branch, never a load.  Everything
// else -- the cells, the order of every sum, the stores -- is tdn_front_kernel's, spelled the same way: the same bits as that
// kernel on the gathered planes.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTdnThreads) tdn_front_pool_kernel(const tsm_host::TdnPoolSource src, float *__restrict__ in4,
                                                                     float *__restrict__ patches, int H, int W) {
  using namespace tsm_host;
  __shared__ __attribute__((aligned(16))) float tile[kPT * kPT * kTdnDiffC];
  const int hp = H / 2, wp = W / 2, ho = H / 4, wo = W / 4;
  const int tiles_x = wo / kTdnTile;
  const int oy0 = (int)(blockIdx.x / tiles_x) * kTdnTile, ox0 = (int)(blockIdx.x % tiles_x) * kTdnTile;
  const int64_t f = blockIdx.y;
  const float *fr[kTdnFrames];   // the segment's five frames, nullptr: planes of zeros
  {
    const int64_t dc = f / src.T;
    const int64_t clip = src.first_clip > INT64_MAX - dc ? INT64_MAX : src.first_clip + dc;
    const int k = (int)(f - dc * src.T);
#pragma unroll
    for (int j = 0; j < kTdnFrames; ++j) {
      const int64_t n = src.mode == 0 ? tdn_table_frame(src.index[f * kTdnFrames + j], src.limit)
                                      : tdn_window_frame(src.first_source_frame, src.total_frames, clip, k, j, src.clip_step,
                                                         src.clip_stride, src.n_frames, src.pad_frame);
      fr[j] = n >= 0 ? src.frames + n * 3 * (int64_t)H * W : nullptr;
    }
  }
  for (int idx = threadIdx.x; idx < kPT * kPT; idx += kTdnThreads) {
    const int ty = idx / kPT, tx = idx - ty * kPT;
    const int py = 2 * oy0 - 3 + ty, px = 2 * ox0 - 3 + tx;
    float p[kTdnDiffC];
#pragma unroll
    for (int c = 0; c < kTdnDiffC; ++c) p[c] = 0.f;
    if (py >= 0 && py < hp && px >= 0 && px < wp) {
      f32x2 v[kTdnPlanes][2];
#pragma unroll
      for (int pl = 0; pl < kTdnPlanes; ++pl)
#pragma unroll
        for (int r = 0; r < 2; ++r) {
          const f32x2 zero = {0.f, 0.f};
          v[pl][r] = fr[pl / 3] ? *reinterpret_cast<const f32x2 *>(fr[pl / 3] + ((int64_t)(pl % 3) * H + 2 * py + r) * W + 2 * px) : zero;
        }
#pragma unroll
      for (int c = 0; c < kTdnDiffC; ++c) {
        const f32x2 d0 = v[c + 3][0] - v[c][0], d1 = v[c + 3][1] - v[c][1];
        p[c] = ((d0[0] + d0[1]) + (d1[0] + d1[1])) * 0.25f;
      }
      if (ty >= 3 && ty < 3 + 2 * kTdnTile && tx >= 3 && tx < 3 + 2 * kTdnTile) {
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
          for (int q = 0; q < 2; ++q) {
            const f32x4 px4 = {v[6][r][q], v[7][r][q], v[8][r][q], 0.f};
            *reinterpret_cast<f32x4 *>(in4 + ((f * H + 2 * py + r) * W + 2 * px + q) * 4) = px4;
          }
      }
    }
#pragma unroll
    for (int c4 = 0; c4 < kTdnDiffC / 4; ++c4) {
      const f32x4 o = {p[4 * c4], p[4 * c4 + 1], p[4 * c4 + 2], p[4 * c4 + 3]};
      *reinterpret_cast<f32x4 *>(tile + idx * kTdnDiffC + 4 * c4) = o;
    }
  }
  __syncthreads();
  // a thread keeps its K quad for all 64 rows: one row (4 KB) per pass of the workgroup
  const int k = 4 * (int)threadIdx.x;
  const bool real = k < kTdnPatchReal;
  const int ky = k / (7 * kTdnDiffC), rem = k - ky * (7 * kTdnDiffC);
  for (int row = 0; row < kTdnTile * kTdnTile; ++row) {
    const int oyl = row / kTdnTile, oxl = row - oyl * kTdnTile;
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
    if (real) o = *reinterpret_cast<const f32x4 *>(tile + ((2 * oyl + ky) * kPT + 2 * oxl) * kTdnDiffC + rem);
    *reinterpret_cast<f32x4 *>(patches + ((f * ho + oy0 + oyl) * wo + ox0 + oxl) * kTdnPatchK + k) = o;
  }
}

// ---------------------------------------------------------------------------------------------
// tdn_fuse_kernel: x [n, h, w, c] <- alpha x + beta d[n, nearest(y), nearest(x), c], d [n, hd, wd, c]; one channel quad per thread.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tdn_fuse_kernel(float *__restrict__ x, const float *__restrict__ d, int64_t n_quads, int h, int w,
                                                       int hd, int wd, int c4, float alpha, float beta) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_quads; i += stride) {
    const int q = (int)(i % c4);
    int64_t pix = i / c4;
    const int px = (int)(pix % w);
    pix /= w;
    const int py = (int)(pix % h);
    const int64_t f = pix / h;
    const int sy = tsm_host::tdn_nearest(py, hd, h), sx = tsm_host::tdn_nearest(px, wd, w);
    const f32x4 a = *reinterpret_cast<const f32x4 *>(x + i * 4);
    const f32x4 b = *reinterpret_cast<const f32x4 *>(d + (((f * hd + sy) * wd + sx) * c4 + q) * 4);
    *reinterpret_cast<f32x4 *>(x + i * 4) = alpha * a + beta * b;
  }
}

// ---------------------------------------------------------------------------------------------
// tdn_fuse_ring_kernel (TSM_LAYOUT_TDN_RING): tdn_fuse_kernel with its two operands found in a ring of per-segment features.
// x [n, h, w, c] = alpha a[slot] + beta d[slot, nearest(y), nearest(x), c], slot = tdn_ring_slot(table[segment], n_slots), a
// [n_slots, h, w, c], d [n_slots, hd, wd, c]; x is the trunk's own contiguous buffer, so the gather costs no pass of its own: the
// kernel moves the bytes fuse2 moves.  A workgroup walks 256-quad spans, `spans` of them per segment: the segment and its slot
// depend on the span alone, so the table entry is one scalar load per (segment, workgroup) and the slot lives in a scalar
// register; a slot outside the ring is a uniform branch, never a load, and stands for operands of 0.0f.  The same tdn_nearest,
// the same expression alpha * a + beta * b on the same 16-byte operands: tdn_fuse_kernel's bits.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) tdn_fuse_ring_kernel(const float *__restrict__ ring_a, const float *__restrict__ ring_d,
                                                            const int32_t *__restrict__ table, float *__restrict__ x, int64_t n_spans,
                                                            int spans, int32_t n_slots, int h, int w, int hd, int wd, int c4, float alpha,
                                                            float beta) {
  const int64_t seg_quads = (int64_t)h * w * c4, d_quads = (int64_t)hd * wd * c4;
  for (int64_t sp = blockIdx.x; sp < n_spans; sp += gridDim.x) {
    const int64_t seg = sp / spans;
    const int64_t slot = tsm_host::tdn_ring_slot(table[seg], n_slots);
    const int64_t i = (sp - seg * spans) * 256 + threadIdx.x;
    if (i >= seg_quads) continue;
    const int q = (int)(i % c4);
    int64_t pix = i / c4;
    const int px = (int)(pix % w);
    const int py = (int)(pix / w);
    const int sy = tsm_host::tdn_nearest(py, hd, h), sx = tsm_host::tdn_nearest(px, wd, w);
    f32x4 a = {0.f, 0.f, 0.f, 0.f}, b = {0.f, 0.f, 0.f, 0.f};
    if (slot >= 0) {
      a = *reinterpret_cast<const f32x4 *>(ring_a + (slot * seg_quads + i) * 4);
      b = *reinterpret_cast<const f32x4 *>(ring_d + (slot * d_quads + ((int64_t)(sy * wd + sx) * c4 + q)) * 4);
    }
    *reinterpret_cast<f32x4 *>(x + (seg * seg_quads + i) * 4) = alpha * a + beta * b;
  }
}

// ---------------------------------------------------------------------------------------------
// mse_squeeze_kernel<R>: b [M, R] = x [M, 16 R] wq [16 R][R] + bq.  A workgroup stages 256 / R rows of x in LDS (16 KB, one
// contiguous span, 16-byte loads) and a thread owns one output: its row's channels come as LDS broadcasts, the weights as
// consecutive floats over the lanes of a row.  Four partial sums over c mod 4, then ((a0 + a1) + (a2 + a3)) + bias.
// ---------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(kTdnThreads) mse_squeeze_kernel(const float *__restrict__ x, const float *__restrict__ wq,
                                                                  const float *__restrict__ bq, float *__restrict__ b, int64_t M) {
  constexpr int C = 16 * R, P = kTdnThreads / R;
  __shared__ __attribute__((aligned(16))) float xs[P * C];
  const int64_t row0 = (int64_t)blockIdx.x * P;
#pragma unroll
  for (int i = 0; i < P * C / 4 / kTdnThreads; ++i) {
    const int q = i * kTdnThreads + threadIdx.x;
    const int64_t row = row0 + q / (C / 4);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < M) v = *reinterpret_cast<const f32x4 *>(x + row0 * C + (int64_t)q * 4);
    *reinterpret_cast<f32x4 *>(xs + q * 4) = v;
  }
  __syncthreads();
  const int p = threadIdx.x / R, j = threadIdx.x % R;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
  for (int c = 0; c < C; c += 4) {
    const f32x4 v = *reinterpret_cast<const f32x4 *>(xs + p * C + c);
    a0 = fmaf(v[0], wq[(c + 0) * R + j], a0);
    a1 = fmaf(v[1], wq[(c + 1) * R + j], a1);
    a2 = fmaf(v[2], wq[(c + 2) * R + j], a2);
    a3 = fmaf(v[3], wq[(c + 3) * R + j], a3);
  }
  if (row0 + p < M) b[(row0 + p) * R + j] = ((a0 + a1) + (a2 + a3)) + bq[j];
}

// ---------------------------------------------------------------------------------------------
// mse_diff_kernel<R>.  b [N, H, W, R], N = n_clips * T.  One thread per frame, 2 x 2 pixel cell and channel quad.  Per direction
// it reads the 4 x 4 neighbourhood of the cell in the neighbouring frame (zero outside the map: the depthwise conv's padding),
// forms c at the cell's four pixels and stores d = c - b[t] there, and the cell's average ((d00 + d01) + (d10 + d11)) / 4 into
// the pooled map [N, H / 2, W / 2, R] when the cell is whole (floor mode).  At the clip's last frame d+ and its pool are written
// as zeros, at its first d- are: frames of another clip are never read.
// ---------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256) mse_diff_kernel(const float *__restrict__ b, const float *__restrict__ dw, float *__restrict__ df,
                                                       float *__restrict__ db, float *__restrict__ pf, float *__restrict__ pb,
                                                       int64_t n_threads, int T, int H, int W) {
  constexpr int Q = R / 4;
  const int ch = (H + 1) / 2, cw = (W + 1) / 2, hp = H / 2, wp = W / 2;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_threads; i += stride) {
    const int q = (int)(i % Q);
    int64_t cell = i / Q;
    const int cx = (int)(cell % cw);
    cell /= cw;
    const int cy = (int)(cell % ch);
    const int64_t n = cell / ch;
    const int t = (int)(n % T);
    f32x4 wk[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) wk[k] = *reinterpret_cast<const f32x4 *>(dw + k * R + 4 * q);
    f32x4 own[2][2];
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int xx = 0; xx < 2; ++xx) {
        own[y][xx] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (2 * cy + y < H && 2 * cx + xx < W) own[y][xx] = *reinterpret_cast<const f32x4 *>(b + ((n * H + 2 * cy + y) * W + 2 * cx + xx) * R + 4 * q);
      }
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      float *d = dir ? db : df, *pool = dir ? pb : pf;
      const bool has = dir ? t > 0 : t < T - 1;
      const int64_t nn = dir ? n - 1 : n + 1;
      f32x4 out[2][2];
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int xx = 0; xx < 2; ++xx) out[y][xx] = f32x4{0.f, 0.f, 0.f, 0.f};
      if (has) {
        f32x4 nb[4][4];
#pragma unroll
        for (int y = 0; y < 4; ++y)
#pragma unroll
          for (int xx = 0; xx < 4; ++xx) {
            const int yy = 2 * cy - 1 + y, xc = 2 * cx - 1 + xx;
            nb[y][xx] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (yy >= 0 && yy < H && xc >= 0 && xc < W) nb[y][xx] = *reinterpret_cast<const f32x4 *>(b + ((nn * H + yy) * W + xc) * R + 4 * q);
          }
#pragma unroll
        for (int y = 0; y < 2; ++y)
#pragma unroll
          for (int xx = 0; xx < 2; ++xx) {
            f32x4 c = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
              for (int kx = 0; kx < 3; ++kx) c += wk[ky * 3 + kx] * nb[y + ky][xx + kx];
            out[y][xx] = c - own[y][xx];
          }
      }
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int xx = 0; xx < 2; ++xx)
          if (2 * cy + y < H && 2 * cx + xx < W) *reinterpret_cast<f32x4 *>(d + ((n * H + 2 * cy + y) * W + 2 * cx + xx) * R + 4 * q) = out[y][xx];
      if (cy < hp && cx < wp)
        *reinterpret_cast<f32x4 *>(pool + ((n * hp + cy) * wp + cx) * R + 4 * q) = ((out[0][0] + out[0][1]) + (out[1][0] + out[1][1])) * 0.25f;
    }
  }
}

// A full 3x3 conv R -> R (padding 1) at pixel (y, x) of frame n, output channel j, for both directions at once: the taps in
// (ky, kx) order, the input channels ascending inside a tap; k [9][R in][R out] carries the BatchNorm scale.
template <int R>
__device__ __forceinline__ void conv3x3_rr(const float *__restrict__ sf, const float *__restrict__ sb, const float *__restrict__ k, int64_t n,
                                           int y, int x, int H, int W, int j, float *af, float *ab) {
  float accf = 0.f, accb = 0.f;
#pragma unroll
  for (int ky = 0; ky < 3; ++ky)
#pragma unroll
    for (int kx = 0; kx < 3; ++kx) {
      const int yy = y - 1 + ky, xx = x - 1 + kx;
      if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
      const int64_t off = ((n * H + yy) * W + xx) * R;
      const float *kt = k + (ky * 3 + kx) * R * R + j;
#pragma unroll
      for (int i = 0; i < R; i += 4) {
        const f32x4 vf = *reinterpret_cast<const f32x4 *>(sf + off + i), vb = *reinterpret_cast<const f32x4 *>(sb + off + i);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float w = kt[(i + e) * R];
          accf = fmaf(vf[e], w, accf);
          accb = fmaf(vb[e], w, accb);
        }
      }
    }
  *af = accf;
  *ab = accb;
}

// ---------------------------------------------------------------------------------------------
// mse_s2_kernel<R>: s2 [N, hp, wp, R] = K2 * pooled d + bias, both directions; one thread per output element.
// ---------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256) mse_s2_kernel(const float *__restrict__ pf, const float *__restrict__ pb, const float *__restrict__ k2,
                                                     const float *__restrict__ b2, float *__restrict__ sf, float *__restrict__ sb,
                                                     int64_t n_out, int hp, int wp) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
    const int j = (int)(i % R);
    int64_t pix = i / R;
    const int x = (int)(pix % wp);
    pix /= wp;
    const int y = (int)(pix % hp);
    float af, ab;
    conv3x3_rr<R>(pf, pb, k2, pix / hp, y, x, hp, wp, j, &af, &ab);
    sf[i] = af + b2[j];
    sb[i] = ab + b2[j];
  }
}

// ---------------------------------------------------------------------------------------------
// mse_mix_kernel<R>: m [N, H, W, R] = d / 3 + s2[nearest] / 3 + (K4 * d + bias) / 3, both directions; one thread per output
// element.  The zero frame of a direction goes through the same arithmetic: the BatchNorm biases make its m non-zero.
// ---------------------------------------------------------------------------------------------
template <int R>
__global__ void __launch_bounds__(256) mse_mix_kernel(const float *__restrict__ df, const float *__restrict__ db, const float *__restrict__ s2f,
                                                      const float *__restrict__ s2b, const float *__restrict__ k4, const float *__restrict__ b4,
                                                      float *__restrict__ mf, float *__restrict__ mb, int64_t n_out, int H, int W) {
  const int hp = H / 2, wp = W / 2;
  const float third = 1.0f / 3.0f;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_out; i += stride) {
    const int j = (int)(i % R);
    int64_t pix = i / R;
    const int x = (int)(pix % W);
    pix /= W;
    const int y = (int)(pix % H);
    const int64_t n = pix / H;
    float af, ab;
    conv3x3_rr<R>(df, db, k4, n, y, x, H, W, j, &af, &ab);
    const int64_t up = ((n * hp + tsm_host::tdn_nearest(y, hp, H)) * wp + tsm_host::tdn_nearest(x, wp, W)) * R + j;
    mf[i] = (third * df[i] + third * s2f[up]) + third * (af + b4[j]);
    mb[i] = (third * db[i] + third * s2b[up]) + third * (ab + b4[j]);
  }
}

// ---------------------------------------------------------------------------------------------
// mse_excite_shift_kernel<C>.  x [n_clips * T, HW, C] (conv1's output), m+ / m- [n_clips * T, HW, R], R = C / 16; o like x.
// A lane owns one pixel and four channels: its four rows of W3 [C][R] stay in registers (4 R floats), the C / 4 lanes of a pixel
// read its m rows as broadcasts.  It walks the clip's T frames once: at step t it forms g[t + 1] = x + x y from x[t + 1] and
// m[t + 1], holds g[t - 1], g[t], g[t + 1] and stores o[t] = (w0 g[t - 1] + w1 g[t]) + w2 g[t + 1], zeros beyond the clip's
// ends.  Every x and o element moves once, 16 bytes per lane.
// ---------------------------------------------------------------------------------------------
template <int C>
__global__ void __launch_bounds__(kTdnThreads) mse_excite_shift_kernel(const float *__restrict__ x, const float *__restrict__ mf,
                                                                       const float *__restrict__ mb, const float *__restrict__ w3,
                                                                       const float *__restrict__ b3, const float *__restrict__ wt,
                                                                       float *__restrict__ o, int T, int HW) {
  constexpr int R = C / 16, L = C / 4, PPB = kTdnThreads / L;
  const int c0 = (threadIdx.x % L) * 4;
  int p = (int)blockIdx.x * PPB + threadIdx.x / L;
  const bool live = p < HW;
  if (!live) p = HW - 1;
  const int64_t clip = blockIdx.y;
  f32x4 wr[4][R / 4];
#pragma unroll
  for (int e = 0; e < 4; ++e)
#pragma unroll
    for (int i = 0; i < R / 4; ++i) wr[e][i] = *reinterpret_cast<const f32x4 *>(w3 + (c0 + e) * R + 4 * i);
  const f32x4 bias = *reinterpret_cast<const f32x4 *>(b3 + c0);
  const f32x4 w0 = *reinterpret_cast<const f32x4 *>(wt + c0), w1 = *reinterpret_cast<const f32x4 *>(wt + C + c0),
              w2 = *reinterpret_cast<const f32x4 *>(wt + 2 * C + c0);
  const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
  f32x4 gm = zero, g0 = zero;
  for (int t = -1; t < T; ++t) {
    f32x4 gp = zero;
    if (t + 1 < T) {
      const int64_t row = (clip * T + t + 1) * HW + p;
      const f32x4 xv = *reinterpret_cast<const f32x4 *>(x + row * C + c0);
      f32x4 ef = bias, eb = bias;
#pragma unroll
      for (int i = 0; i < R / 4; ++i) {
        const f32x4 vf = *reinterpret_cast<const f32x4 *>(mf + row * R + 4 * i), vb = *reinterpret_cast<const f32x4 *>(mb + row * R + 4 * i);
#pragma unroll
        for (int ii = 0; ii < 4; ++ii)
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            ef[e] = fmaf(wr[e][i][ii], vf[ii], ef[e]);
            eb[e] = fmaf(wr[e][i][ii], vb[ii], eb[e]);
          }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float yf = 1.0f / (1.0f + expf(-ef[e])) - 0.5f, yb = 1.0f / (1.0f + expf(-eb[e])) - 0.5f;
        const float y = 0.5f * yf + 0.5f * yb;
        gp[e] = xv[e] + xv[e] * y;
      }
    }
    if (t >= 0 && live) *reinterpret_cast<f32x4 *>(o + ((clip * T + t) * HW + p) * C + c0) = (w0 * gm + w1 * g0) + w2 * gp;
    gm = g0;
    g0 = gp;
  }
}

static bool mse_width_ok(int c) { return c == 128 || c == 256 || c == 512; }

// What both front-end launches check: grid y = segments (at most 65535), grid x = 8 x 8 tiles of conv1_5 outputs; 0: refused.
static int64_t tdn_front_tiles(const float *in4, const float *patches, int n_segments, int h, int w) {
  if (!in4 || !patches || n_segments <= 0 || n_segments > 65535 || h < 64 || w < 64 || h % 32 != 0 || w % 32 != 0) return 0;
  const int64_t tiles = (int64_t)(h / 4 / tsm_host::kTdnTile) * (w / 4 / tsm_host::kTdnTile);
  return tiles > 0x7fffffffL ? 0 : tiles;
}

hipError_t launch_tdn_front(const float *x, float *in4, float *patches, int n_frames, int h, int w, hipStream_t s) {
  const int64_t tiles = tdn_front_tiles(in4, patches, n_frames, h, w);
  if (!x || !tiles) return hipErrorInvalidValue;
  TSM_KLAUNCH(tdn_front_kernel, dim3((unsigned)tiles, (unsigned)n_frames), dim3(kTdnThreads), 0, s, x, in4, patches, h, w);
  return hipGetLastError();
}

hipError_t launch_tdn_front_pool(const tsm_host::TdnPoolSource &src, float *in4, float *patches, int n_segments, int h, int w, hipStream_t s) {
  if (!src.frames || reinterpret_cast<uintptr_t>(src.frames) % 8 != 0 || src.n_frames <= 0 || (src.mode != 0 && src.mode != 1) ||
      (src.mode == 0 && !src.index) || src.T <= 0 || src.limit != tsm_host::tdn_table_limit(src.n_frames))
    return hipErrorInvalidValue;
  const int64_t tiles = tdn_front_tiles(in4, patches, n_segments, h, w);
  if (!tiles) return hipErrorInvalidValue;
  TSM_KLAUNCH(tdn_front_pool_kernel, dim3((unsigned)tiles, (unsigned)n_segments), dim3(kTdnThreads), 0, s, src, in4, patches, h, w);
  return hipGetLastError();
}

hipError_t launch_tdn_fuse(float *x, const float *d, int n, int h, int w, int hd, int wd, int c, float alpha, float beta, hipStream_t s) {
  if (!x || !d || n <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0 || c <= 0 || c % 4 != 0) return hipErrorInvalidValue;
  const int64_t quads = (int64_t)n * h * w * (c / 4);
  TSM_KLAUNCH(tdn_fuse_kernel, dim3(grid_for(quads, 16384)), dim3(256), 0, s, x, d, quads, h, w, hd, wd, c / 4, alpha, beta);
  return hipGetLastError();
}

// n segments of the trunk's buffer x from the ring; the launch cap is tdn_fuse_kernel's (16384 workgroups of 256 quads).
hipError_t launch_tdn_fuse_ring(const float *ring_a, const float *ring_d, const int32_t *table, int n_slots, float *x, int n, int h, int w,
                                int hd, int wd, int c, float alpha, float beta, hipStream_t s) {
  if (!ring_a || !ring_d || !table || !x || n_slots <= 0 || n <= 0 || h <= 0 || w <= 0 || hd <= 0 || wd <= 0 || c <= 0 || c % 4 != 0)
    return hipErrorInvalidValue;
  const int64_t seg_quads = (int64_t)h * w * (c / 4), spans = (seg_quads + 255) / 256;
  if (spans > 0x7fffffffL) return hipErrorInvalidValue;
  const int64_t n_spans = spans * n;
  TSM_KLAUNCH(tdn_fuse_ring_kernel, dim3(grid_for(n_spans * 256, 16384)), dim3(256), 0, s, ring_a, ring_d, table, x, n_spans, (int)spans,
              n_slots, h, w, hd, wd, c / 4, alpha, beta);
  return hipGetLastError();
}

hipError_t launch_mse_squeeze(const float *x, const float *wq, const float *bq, float *b, int64_t m, int c, hipStream_t s) {
  if (!x || !wq || !bq || !b || m <= 0 || !mse_width_ok(c)) return hipErrorInvalidValue;
  const int r = c / tsm_host::kTdnReduction;
  const int64_t blocks = (m + kTdnThreads / r - 1) / (kTdnThreads / r);
  if (blocks > 0x7fffffffL) return hipErrorInvalidValue;
#define TSM_SQ(RR) TSM_KLAUNCH(mse_squeeze_kernel<RR>, dim3((unsigned)blocks), dim3(kTdnThreads), 0, s, x, wq, bq, b, m)
  if (r == 8) TSM_SQ(8);
  else if (r == 16) TSM_SQ(16);
  else TSM_SQ(32);
#undef TSM_SQ
  return hipGetLastError();
}

hipError_t launch_mse_diff(const float *b, const float *dw, float *df, float *db, float *pf, float *pb, int n_frames, int T, int h, int w,
                           int c, hipStream_t s) {
  if (!b || !dw || !df || !db || !pf || !pb || n_frames <= 0 || T < 2 || n_frames % T != 0 || h < 2 || w < 2 || !mse_width_ok(c)) return hipErrorInvalidValue;
  const int r = c / tsm_host::kTdnReduction;
  const int64_t threads = (int64_t)n_frames * ((h + 1) / 2) * ((w + 1) / 2) * (r / 4);
#define TSM_DF(RR) TSM_KLAUNCH(mse_diff_kernel<RR>, dim3(grid_for(threads, 16384)), dim3(256), 0, s, b, dw, df, db, pf, pb, threads, T, h, w)
  if (r == 8) TSM_DF(8);
  else if (r == 16) TSM_DF(16);
  else TSM_DF(32);
#undef TSM_DF
  return hipGetLastError();
}

hipError_t launch_mse_s2(const float *pf, const float *pb, const float *k2, const float *b2, float *sf, float *sb, int n_frames, int hp, int wp,
                         int c, hipStream_t s) {
  if (!pf || !pb || !k2 || !b2 || !sf || !sb || n_frames <= 0 || hp <= 0 || wp <= 0 || !mse_width_ok(c)) return hipErrorInvalidValue;
  const int r = c / tsm_host::kTdnReduction;
  const int64_t outs = (int64_t)n_frames * hp * wp * r;
#define TSM_S2(RR) TSM_KLAUNCH(mse_s2_kernel<RR>, dim3(grid_for(outs, 16384)), dim3(256), 0, s, pf, pb, k2, b2, sf, sb, outs, hp, wp)
  if (r == 8) TSM_S2(8);
  else if (r == 16) TSM_S2(16);
  else TSM_S2(32);
#undef TSM_S2
  return hipGetLastError();
}

hipError_t launch_mse_mix(const float *df, const float *db, const float *s2f, const float *s2b, const float *k4, const float *b4, float *mf,
                          float *mb, int n_frames, int h, int w, int c, hipStream_t s) {
  if (!df || !db || !s2f || !s2b || !k4 || !b4 || !mf || !mb || n_frames <= 0 || h < 2 || w < 2 || !mse_width_ok(c)) return hipErrorInvalidValue;
  const int r = c / tsm_host::kTdnReduction;
  const int64_t outs = (int64_t)n_frames * h * w * r;
#define TSM_MX(RR) TSM_KLAUNCH(mse_mix_kernel<RR>, dim3(grid_for(outs, 16384)), dim3(256), 0, s, df, db, s2f, s2b, k4, b4, mf, mb, outs, h, w)
  if (r == 8) TSM_MX(8);
  else if (r == 16) TSM_MX(16);
  else TSM_MX(32);
#undef TSM_MX
  return hipGetLastError();
}

hipError_t launch_mse_excite_shift(const float *x, const float *mf, const float *mb, const float *w3, const float *b3, const float *wt, float *o,
                                   int n_clips, int T, int hw, int c, hipStream_t s) {
  if (!x || !mf || !mb || !w3 || !b3 || !wt || !o || n_clips <= 0 || n_clips > 65535 || T < 1 || hw <= 0 || !mse_width_ok(c)) return hipErrorInvalidValue;
  const int ppb = kTdnThreads / (c / 4);
  const dim3 grid((unsigned)((hw + ppb - 1) / ppb), (unsigned)n_clips);
#define TSM_EX(CH) TSM_KLAUNCH(mse_excite_shift_kernel<CH>, grid, dim3(kTdnThreads), 0, s, x, mf, mb, w3, b3, wt, o, T, hw)
  if (c == 128) TSM_EX(128);
  else if (c == 256) TSM_EX(256);
  else TSM_EX(512);
#undef TSM_EX
  return hipGetLastError();
}

}  // namespace tsm
