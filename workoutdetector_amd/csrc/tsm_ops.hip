// Small streaming kernels around the conv stack, and device_info().
#include "tsm_device.h"
#include "tsm_host_util.h"

#include <string>

namespace tsm {

// =============================================================================================
// Storage formats of activations outside the conv kernel.  A "group" is the unit one thread moves:
//   kPrecF32     4 channels, 16 bytes (4 floats)
//   kPrecBf16x3  8 channels, 32 bytes [hi x8 | lo x8] (split-bf16)
//   kPrecBf16    8 channels, 16 bytes (8 bf16)
// Pointers stay float-typed; gf = group size in 4-byte units.
// =============================================================================================
template <int FMT>
struct Fmt {
  static constexpr int ch = FMT == kPrecF32 ? 4 : 8;
  static constexpr int gf = FMT == kPrecBf16x3 ? 8 : 4;
};

template <int FMT>
__device__ __forceinline__ void load_group(const float *p, float v[8]) {
  if (FMT == kPrecF32) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(p);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      v[e] = a[e];
      v[e + 4] = 0.f;
    }
  } else if (FMT == kPrecBf16x3) {
    const u32x4 h = *reinterpret_cast<const u32x4 *>(p), l = *reinterpret_cast<const u32x4 *>(p + 4);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = split_elem(h, e) + split_elem(l, e);
  } else {
    const u32x4 h = *reinterpret_cast<const u32x4 *>(p);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = split_elem(h, e);
  }
}

template <int FMT>
__device__ __forceinline__ void store_group(float *p, const float v[8]) {
  if (FMT == kPrecF32) {
    *reinterpret_cast<f32x4 *>(p) = f32x4{v[0], v[1], v[2], v[3]};
  } else if (FMT == kPrecBf16x3) {
    u32x4 oh, ol;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      unsigned hw, lw;
      split_pair(v[2 * w], v[2 * w + 1], &hw, &lw);
      oh[w] = hw;
      ol[w] = lw;
    }
    *reinterpret_cast<u32x4 *>(p) = oh;
    *reinterpret_cast<u32x4 *>(p + 4) = ol;
  } else {
    u32x4 o;
#pragma unroll
    for (int w = 0; w < 4; ++w) o[w] = pack_bf16(v[2 * w], v[2 * w + 1]);
    *reinterpret_cast<u32x4 *>(p) = o;
  }
}


#define TSM_DISPATCH_FMT(prec, KERNEL, grid, stream, ...)                                                   \
  do {                                                                                                      \
    if ((prec) == kPrecBf16x3)                                                                              \
      TSM_KLAUNCH((KERNEL<kPrecBf16x3>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);             \
    else if ((prec) == kPrecBf16)                                                                           \
      TSM_KLAUNCH((KERNEL<kPrecBf16>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);               \
    else                                                                                                    \
      TSM_KLAUNCH((KERNEL<kPrecF32>), dim3(grid), dim3(256), 0, stream, __VA_ARGS__);                \
  } while (0)

// ---------------------------------------------------------------------------------------------
// pack_input: [N,3,H,W] or [N,H,W,3] fp32 -> the stem's input format, padding channels zero:
//   fp32   one 4-channel group per pixel (NHWC4)
//   bf16 formats   one 8-element group per pixel PAIR: (pixel 2j: c0 c1 c2 0, pixel 2j+1: c0 c1 c2 0), rows of
//                  ceil(W/2) pairs (an odd width ends in a zero pixel, which is what the conv's padding reads anyway)
// One thread per group.
// ---------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(256) pack_input_kernel(const float *__restrict__ src,
                                                         float *__restrict__ dst, int64_t n_groups, int h, int w,
                                                         int nchw) {
  constexpr int PX = FMT == kPrecF32 ? 1 : 2;  // pixels per group
  const int wg = (w + PX - 1) / PX;
  const int64_t hw = (int64_t)h * w;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_groups; i += stride) {
    const int gx = (int)(i % wg);
    const int64_t row = i / wg;  // n * h + y
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < PX; ++q) {
      const int x = gx * PX + q;
      if (x < w) {
        if (nchw) {
          const int64_t n = row / h, y = row - n * h;
          const float *b = src + n * 3 * hw + y * w + x;
          v[4 * q + 0] = b[0];
          v[4 * q + 1] = b[hw];
          v[4 * q + 2] = b[2 * hw];
        } else {
          const float *b = src + (row * w + x) * 3;
          v[4 * q + 0] = b[0];
          v[4 * q + 1] = b[1];
          v[4 * q + 2] = b[2];
        }
      }
    }
    store_group<FMT>(dst + i * Fmt<FMT>::gf, v);
  }
}

hipError_t launch_pack_input(const float *src, float *dst, int64_t n_frames, int h, int w, int nchw, int prec,
                             hipStream_t s) {
  const int wg = prec == kPrecF32 ? w : (w + 1) / 2;
  const int64_t total = n_frames * h * wg;
  TSM_DISPATCH_FMT(prec, pack_input_kernel, grid_for(total, 4096), s, src, dst, total, h, w, nchw);
  return hipGetLastError();
}

// fp32 [n8 * 8] <-> another format, 8 channels per thread
template <int FMT>
__global__ void __launch_bounds__(256) from_f32_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                       int64_t n8) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    const f32x4 a = *reinterpret_cast<const f32x4 *>(x + i * 8), b = *reinterpret_cast<const f32x4 *>(x + i * 8 + 4);
    const float v[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    store_group<FMT>(y + i * Fmt<FMT>::gf, v);
  }
}
template <int FMT>
__global__ void __launch_bounds__(256) to_f32_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                     int64_t n8) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += stride) {
    float v[8];
    load_group<FMT>(x + i * Fmt<FMT>::gf, v);
    *reinterpret_cast<f32x4 *>(y + i * 8) = f32x4{v[0], v[1], v[2], v[3]};
    *reinterpret_cast<f32x4 *>(y + i * 8 + 4) = f32x4{v[4], v[5], v[6], v[7]};
  }
}
hipError_t launch_from_f32(const float *x, float *y, int64_t n8, int prec, hipStream_t s) {
  if (prec == kPrecBf16x3)
    TSM_KLAUNCH(from_f32_kernel<kPrecBf16x3>, dim3(grid_for(n8, 8192)), dim3(256), 0, s, x, y, n8);
  else if (prec == kPrecBf16)
    TSM_KLAUNCH(from_f32_kernel<kPrecBf16>, dim3(grid_for(n8, 8192)), dim3(256), 0, s, x, y, n8);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}
hipError_t launch_to_f32(const float *x, float *y, int64_t n8, int prec, hipStream_t s) {
  if (prec == kPrecBf16x3)
    TSM_KLAUNCH(to_f32_kernel<kPrecBf16x3>, dim3(grid_for(n8, 8192)), dim3(256), 0, s, x, y, n8);
  else if (prec == kPrecBf16)
    TSM_KLAUNCH(to_f32_kernel<kPrecBf16>, dim3(grid_for(n8, 8192)), dim3(256), 0, s, x, y, n8);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Frame transforms: staged raw frames [n,h,w,3] u8|f32, or NV12 [n,3h/2,w] bytes, -> resized, normalised frames in the
// engine's input formats.
// One thread per output group: a pixel (out_mode 0 NHWC4 fp32, 1 NCHW fp32) or a pixel pair (2 split-bf16, 3 bf16: the
// stem's packed-pair input, see pack_input_kernel); neighbouring threads are neighbouring ox: contiguous 16-byte stores.
// preprocess_kernel, preprocess_indexed_kernel, preprocess_clips_kernel and preprocess_windows_kernel are ONE row loop
// (preprocess_rows) over four row sources -- which frame, and which window of it, output row f shows -- and two samplers over
// one bilinear-and-normalise core, which read their taps from a tap source (Taps<T>: RGB u8 | f32, NV12 and five more YUV formats); preprocess_image_kernel
// (Pillow's antialiased resample, further down) shares the constants and the group writer.
// Bilinear sampling follows ATen's CPU kernel (UpSampleBilinear2d, no antialias): src = scale * (dst + 0.5)
// - 0.5 clamped at 0, scale = in / out, out = h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11); then
// (v * pre_scale - mean) / std.  datasets/build.py:123-136 of the reference (torchvision tensor transforms).
// ---------------------------------------------------------------------------------------------
__device__ constexpr float kMean[3] = {0.485f, 0.456f, 0.406f}, kStd[3] = {0.229f, 0.224f, 0.225f};   // Normalize, ImageNet

// The arithmetic of a pixel is spelled out -- contraction off, the fused steps written as fmaf -- so that EVERY inlined copy
// of it computes the same bits: left to the compiler, the second pixel of a pixel pair rounded the other product of each
// bilinear sum (fma(w0, p00, w1 * p01) where the first pixel had fma(w1, p01, w0 * p00)), so a pair layout's odd pixels
// were one fp32 ulp of the interpolated value away from the fp32 layouts' -- after the mean is subtracted, up to 1e-4
// relative on a value near zero.  With one spelling NTHWC8S / NTHWC8B hold the split / the rounding of exactly the numbers
// NTHWC4 and NTCHW hold, in all three kernels, and a whole-frame box equals the centre crop of the same map bit for bit.
__device__ __forceinline__ float sample_coord(float scale, float o) {
#pragma clang fp contract(off)
  const float f = __builtin_fmaf(scale, o + 0.5f, -0.5f);
  return f < 0.f ? 0.f : f;
}
// channel c of one output pixel from its four taps: h0 * (w0 * p00 + w1 * p01) + h1 * (w0 * p10 + w1 * p11), normalised
__device__ __forceinline__ float bilinear_normalised(float p00, float p01, float p10, float p11, float w0, float w1, float h0,
                                                     float h1, float pre_scale, int c) {
#pragma clang fp contract(off)
  // (the two rows as the lanes of one packed multiply and one packed fma: the same two roundings per lane)
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  const f32x2 row = __builtin_elementwise_fma(f32x2{w1, w1}, f32x2{p01, p11}, f32x2{w0, w0} * f32x2{p00, p10});
  const float t = __builtin_fmaf(h1, row[1], h0 * row[0]);
  return __builtin_fmaf(t, pre_scale, -kMean[c]) / kStd[c];
}
// The reference's zero frame after Normalize: the padded tail of a clip, a table entry outside the buffer.
__device__ __forceinline__ void zero_frame_pixel(float *v) {
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = (0.f - kMean[c]) / kStd[c];
}

// One output group (pixel gx, or pixels 2 gx and 2 gx + 1, of row oy of frame f; `g` its running number) to dst.
__device__ __forceinline__ void store_pixel_group(float *dst, int out_mode, int size, int64_t f, int oy, int gx, int64_t g,
                                                  const float v[8]) {
  if (out_mode == 1) {
    float *o = dst + f * 3 * (int64_t)size * size + (int64_t)oy * size + gx;
    o[0] = v[0];
    o[(int64_t)size * size] = v[1];
    o[2 * (int64_t)size * size] = v[2];
  } else if (out_mode == 2) {
    store_group<kPrecBf16x3>(dst + g * 8, v);
  } else if (out_mode == 3) {
    store_group<kPrecBf16>(dst + g * 4, v);
  } else {
    store_group<kPrecF32>(dst + g * 4, v);
  }
}

// Tap sources: the frame a sampler reads.  Taps<T> is one staged frame of a launch; quad() gives the three channel values, as
// floats, of the four taps (y0 | y1, x0 | x1) of a bilinear sample.  Coordinates lie in the frame; a tap whose mask is false
// is RGB 0 (the person crop's zero fill) whatever the frame holds there.
//   * Taps<unsigned char>, Taps<float>: [h, w, 3] of T, three loads per tap.
//   * Taps<Nv12>: h * w luma bytes, then h / 2 rows of w bytes of (U, V) pairs (tsm_host_util.h: the layout, the integer
//     conversion and both offsets are the host's text).  A tap is one luma byte and one aligned 2-byte chroma load (U the low
//     byte); taps of one 2x2 block share a pair, so the second column and the second row load only where they leave the block
//     of the first.  The conversion's three integers in 0 .. 255 become floats exactly as a staged uint8 RGB frame's bytes do.
struct Nv12 {};
template <typename T>
struct Taps {
  const T *frame;
  int w;
  static __device__ __forceinline__ Taps of(const void *base, int64_t j, int h, int w, const int32_t *) {
    return {static_cast<const T *>(base) + j * (int64_t)h * w * 3, w};
  }
  static __device__ __forceinline__ bool descriptor_ok(const int32_t *d, int n_segment, int64_t arena_bytes, bool center, int resize,
                                                       int crop, int64_t *off, tsm_host::CropGeometry *g) {
    return tsm_host::window_descriptor_ok(d, n_segment, (int)sizeof(T), arena_bytes, center, resize, crop, off, g);
  }
  __device__ __forceinline__ void quad(int64_t y0, int64_t y1, int64_t x0, int64_t x1, bool m00, bool m01, bool m10, bool m11,
                                       float t[4][3]) const {
    const T *r0 = frame + y0 * w * 3, *r1 = frame + y1 * w * 3;
    const T *a00 = r0 + x0 * 3, *a01 = r0 + x1 * 3, *a10 = r1 + x0 * 3, *a11 = r1 + x1 * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      t[0][c] = m00 ? (float)a00[c] : 0.f;
      t[1][c] = m01 ? (float)a01[c] : 0.f;
      t[2][c] = m10 ? (float)a10[c] : 0.f;
      t[3][c] = m11 ? (float)a11[c] : 0.f;
    }
  }
  // one pixel's three channels as integers (the image path: Pillow's 8-bit resample); 8-bit frames only
  __device__ __forceinline__ void pixel(int64_t y, int64_t x, unsigned rgb[3]) const {
    const T *a = frame + (y * w + x) * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = (unsigned)a[c];
  }
};
template <>
struct Taps<Nv12> {
  const unsigned char *frame;
  int h, w;
  tsm_host::Nv12Coef k;
  static __device__ __forceinline__ Taps of(const void *base, int64_t j, int h, int w, const int32_t *coef) {
    return {static_cast<const unsigned char *>(base) + j * ((int64_t)h * w / 2 * 3), h, w, tsm_host::nv12_coef_of(coef)};
  }
  static __device__ __forceinline__ bool descriptor_ok(const int32_t *d, int n_segment, int64_t arena_bytes, bool center, int resize,
                                                       int crop, int64_t *off, tsm_host::CropGeometry *g) {
    return tsm_host::nv12_window_descriptor_ok(d, n_segment, arena_bytes, center, resize, crop, off, g);
  }
  __device__ __forceinline__ unsigned pair(int64_t y, int64_t x) const {
    return *reinterpret_cast<const unsigned short *>(frame + tsm_host::nv12_chroma_offset(h, w, y, x));
  }
  __device__ __forceinline__ void tap(int64_t y, int64_t x, unsigned uv, bool m, float *t) const {
    int rgb[3];
    tsm_host::nv12_pixel_rgb(k, frame[tsm_host::nv12_luma_offset(w, y, x)], (int)(uv & 255u), (int)(uv >> 8), rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = m ? (float)rgb[c] : 0.f;
  }
  __device__ __forceinline__ void quad(int64_t y0, int64_t y1, int64_t x0, int64_t x1, bool m00, bool m01, bool m10, bool m11,
                                       float t[4][3]) const {
    const bool new_col = (x1 >> 1) != (x0 >> 1), new_row = (y1 >> 1) != (y0 >> 1);
    const unsigned uv00 = pair(y0, x0);
    unsigned uv01 = uv00;
    if (new_col) uv01 = pair(y0, x1);
    unsigned uv10 = uv00, uv11 = uv01;
    if (new_row) {
      uv10 = pair(y1, x0);
      uv11 = uv10;
      if (new_col) uv11 = pair(y1, x1);
    }
    tap(y0, x0, uv00, m00, t[0]);
    tap(y0, x1, uv01, m01, t[1]);
    tap(y1, x0, uv10, m10, t[2]);
    tap(y1, x1, uv11, m11, t[3]);
  }
  // one pixel as integers: one luma byte and one aligned 2-byte chroma load, then the conversion
  __device__ __forceinline__ void pixel(int64_t y, int64_t x, unsigned rgb[3]) const {
    const unsigned uv = pair(y, x);
    int v[3];
    tsm_host::nv12_pixel_rgb(k, frame[tsm_host::nv12_luma_offset(w, y, x)], (int)(uv & 255u), (int)(uv >> 8), v);
#pragma unroll
    for (int c = 0; c < 3; ++c) rgb[c] = (unsigned)v[c];
  }
};

// The other YUV sources (tsm_host_util.h: YuvLayout, the offsets and the descriptor rule are the host's text), one
// specialisation per format over one body, YuvTaps<Tag>: the layout is a compile-time constant, so every offset folds to the
// address arithmetic of that format alone and a launch pays for no format but its own.  Taps that share their chroma load
// it once, as Taps<Nv12>'s do; `group` is what they share:
//   * I420, Yv12: one U byte and one V byte per 2x2 block (two byte loads), luma one byte per tap.
//   * P010: one aligned 4-byte load per 2x2 block holds the U and the V word; luma is the high byte of its word, one byte per tap.
//   * Yuyv, Uyvy: one aligned 4-byte load per pixel pair holds both luma bytes, U and V: a tap needs no load of its own.
//     Rows share nothing (4:2:2), so the second row loads again unless it is the first (a tap clamped at the border).
struct I420 { static constexpr int kLayout = tsm_host::kYuvI420; };
struct Yv12 { static constexpr int kLayout = tsm_host::kYuvYv12; };
struct P010 { static constexpr int kLayout = tsm_host::kYuvP010; };
struct Yuyv { static constexpr int kLayout = tsm_host::kYuvYuyv; };
struct Uyvy { static constexpr int kLayout = tsm_host::kYuvUyvy; };
template <typename Tag>
struct YuvTaps {
  static constexpr int L = Tag::kLayout;
  static constexpr bool kPlanar = L == tsm_host::kYuvI420 || L == tsm_host::kYuvYv12;
  static constexpr bool kPacked = L == tsm_host::kYuvYuyv || L == tsm_host::kYuvUyvy;
  const unsigned char *frame;
  int h, w;
  tsm_host::Nv12Coef k;
  static __device__ __forceinline__ YuvTaps of(const void *base, int64_t j, int h, int w, const int32_t *coef) {
    return {static_cast<const unsigned char *>(base) + j * tsm_host::yuv_frame_bytes(L, h, w), h, w, tsm_host::nv12_coef_of(coef)};
  }
  static __device__ __forceinline__ bool descriptor_ok(const int32_t *d, int n_segment, int64_t arena_bytes, bool center, int resize,
                                                       int crop, int64_t *off, tsm_host::CropGeometry *g) {
    return tsm_host::yuv_window_descriptor_ok(L, d, n_segment, arena_bytes, center, resize, crop, off, g);
  }
  // what the taps of one chroma group share: (U | V << 8) of the planar layouts, the aligned 4 bytes of the others
  __device__ __forceinline__ unsigned group(int64_t y, int64_t x) const {
    if constexpr (kPlanar)
      return (unsigned)frame[tsm_host::yuv_u_offset(L, h, w, y, x)] | ((unsigned)frame[tsm_host::yuv_v_offset(L, h, w, y, x)] << 8);
    else
      return *reinterpret_cast<const unsigned *>(frame + tsm_host::yuv_group_offset(L, h, w, y, x));
  }
  __device__ __forceinline__ void tap(int64_t y, int64_t x, unsigned g, bool m, float *t) const {
    int Y, U, V;
    if constexpr (kPlanar) {
      Y = frame[tsm_host::yuv_y_offset(L, h, w, y, x)]; U = (int)(g & 255u); V = (int)(g >> 8);
    } else if constexpr (L == tsm_host::kYuvP010) {
      Y = frame[tsm_host::yuv_y_offset(L, h, w, y, x)]; U = (int)((g >> 8) & 255u); V = (int)(g >> 24);
    } else if constexpr (L == tsm_host::kYuvYuyv) {
      Y = (int)((g >> (((unsigned)x & 1u) << 4)) & 255u); U = (int)((g >> 8) & 255u); V = (int)(g >> 24);
    } else {
      Y = (int)((g >> ((((unsigned)x & 1u) << 4) + 8)) & 255u); U = (int)(g & 255u); V = (int)((g >> 16) & 255u);
    }
    int rgb[3];
    tsm_host::nv12_pixel_rgb(k, Y, U, V, rgb);
#pragma unroll
    for (int c = 0; c < 3; ++c) t[c] = m ? (float)rgb[c] : 0.f;
  }
  __device__ __forceinline__ void quad(int64_t y0, int64_t y1, int64_t x0, int64_t x1, bool m00, bool m01, bool m10, bool m11,
                                       float t[4][3]) const {
    const bool new_col = (x1 >> 1) != (x0 >> 1), new_row = kPacked ? y1 != y0 : (y1 >> 1) != (y0 >> 1);
    const unsigned g00 = group(y0, x0);
    unsigned g01 = g00;
    if (new_col) g01 = group(y0, x1);
    unsigned g10 = g00, g11 = g01;
    if (new_row) {
      g10 = group(y1, x0);
      g11 = g10;
      if (new_col) g11 = group(y1, x1);
    }
    tap(y0, x0, g00, m00, t[0]);
    tap(y0, x1, g01, m01, t[1]);
    tap(y1, x0, g10, m10, t[2]);
    tap(y1, x1, g11, m11, t[3]);
  }
};
#define TSM_YUV_TAPS(Tag)                                                          \
  template <>                                                                      \
  struct Taps<Tag> : YuvTaps<Tag> {                                                \
    Taps() = default;                                                              \
    __device__ __forceinline__ Taps(const YuvTaps<Tag> &b) : YuvTaps<Tag>(b) {}    \
  }
TSM_YUV_TAPS(I420);
TSM_YUV_TAPS(Yv12);
TSM_YUV_TAPS(P010);
TSM_YUV_TAPS(Yuyv);
TSM_YUV_TAPS(Uyvy);
#undef TSM_YUV_TAPS

// The row loop.  A row source has a `Row` (where a row's pixels come from), locate(f, &row) -- false: the row has no frame
// and is the zero frame -- and pixel(row, oy, ox, v), its sampler.  Sources are passed by value and inlined.
template <typename Source>
__device__ __forceinline__ void preprocess_rows(float *dst, int out_mode, int size, int64_t n_rows, const Source src) {
  const int px = out_mode >= 2 ? 2 : 1;
  const int wg = (size + px - 1) / px;
  const int64_t per_frame = (int64_t)wg * size;
  const int64_t total = n_rows * per_frame;
  // (256 = the block size of every launch, TSM_LAUNCH_ROWS: read as blockDim.x in here it costs a vector load and a wait at
  //  the head of the kernel, which the scalar load of a kernel's own blockDim.x does not)
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += stride) {
    const int gx = (int)(i % wg);
    const int oy = (int)((i / wg) % size);
    const int64_t f = i / per_frame;
    const bool pair = px == 2 && gx * 2 + 1 < size;      // (an odd size ends in a half-filled pair: the second pixel stays 0)
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    typename Source::Row row;
    if (src.locate(f, &row)) {
      src.pixel(row, oy, gx * px, v);
      if (pair) src.pixel(row, oy, gx * 2 + 1, v + 4);
    } else {
      zero_frame_pixel(v);
      if (pair) zero_frame_pixel(v + 4);
    }
    store_pixel_group(dst, out_mode, size, f, oy, gx, i, v);
  }
}

// preprocess (K8): Resize(int) + CenterCrop.  The sampler of the centre-crop sources: every tap lies in the frame (the
// launcher checks the crop window against the resized size), so nothing is masked.
template <typename T>
__device__ __forceinline__ void preprocess_pixel(const PreprocParams &p, const Taps<T> &frame, int cy, int cx, float *v) {
#pragma clang fp contract(off)
  const float fy = sample_coord((float)p.h / (float)p.nh, (float)(cy + p.top));
  const float fx = sample_coord((float)p.w / (float)p.nw, (float)(cx + p.left));
  const int y0 = (int)fy, x0 = (int)fx;
  const int y1 = y0 + (y0 < p.h - 1 ? 1 : 0), x1 = x0 + (x0 < p.w - 1 ? 1 : 0);
  const float h1 = fy - (float)y0, h0 = 1.f - h1, w1 = fx - (float)x0, w0 = 1.f - w1;
  float t[4][3];
  frame.quad(y0, y1, x0, x1, true, true, true, true, t);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = bilinear_normalised(t[0][c], t[1][c], t[2][c], t[3][c], w0, w1, h0, h1, p.pre_scale, c);
}

// row f is frame f
template <typename T>
struct FrameRows {
  const PreprocParams &p;
  using Row = Taps<T>;
  __device__ __forceinline__ bool locate(int64_t f, Row *frame) const {
    *frame = Taps<T>::of(p.src, f, p.h, p.w, p.nv12);
    return true;
  }
  __device__ __forceinline__ void pixel(const Row &frame, int oy, int ox, float *v) const { preprocess_pixel<T>(p, frame, oy, ox, v); }
};

template <typename T>
__global__ void __launch_bounds__(256) preprocess_kernel(const PreprocParams p) {
  preprocess_rows(p.dst, p.out_mode, p.crop, p.n, FrameRows<T>{p});
}

// The crop window of a centre-crop launch lies in the resized frame (PreprocParams, ImagePreprocParams).
template <typename P>
static bool crop_window_ok(const P &p) {
  return p.h > 0 && p.w > 0 && p.crop > 0 && p.top >= 0 && p.left >= 0 && p.top + p.crop <= p.nh && p.left + p.crop <= p.nw;
}

// YUV frames of a launch whose size the host knows (src_yuv of the parameter blocks).  NV12: both sides even, the buffer
// 2-byte aligned (the chroma pair is one load); the other formats: their layout's parity and alignment.
static bool yuv_frames_ok(int src_yuv, const void *src, int h, int w) {
  if (src_yuv >= 2)
    return tsm_host::yuv_sides_ok(src_yuv - 2, h, w) && (reinterpret_cast<uintptr_t>(src) & (uintptr_t)(tsm_host::yuv_alignment(src_yuv - 2) - 1)) == 0;
  return !src_yuv || (((h | w) & 1) == 0 && (reinterpret_cast<uintptr_t>(src) & 1) == 0);
}

// One grid-stride launch of a row-loop kernel covers any number of rows (64-bit group index): nothing of the launch geometry
// limits a range of clips or a table.
#define TSM_LAUNCH_ROWS(KERNEL, is_u8, src_yuv, n_rows, size, out_mode, stream, params)                    \
  do {                                                                                                      \
    const int px_ = (out_mode) >= 2 ? 2 : 1;                                                                \
    const unsigned grid_ = grid_for((int64_t)(n_rows) * (size) * (((size) + px_ - 1) / px_), 8192);         \
    switch (src_yuv) {                                                                                      \
      case 1: TSM_KLAUNCH(KERNEL<Nv12>, dim3(grid_), dim3(256), 0, stream, params); break;                  \
      case 2 + tsm_host::kYuvI420: TSM_KLAUNCH(KERNEL<I420>, dim3(grid_), dim3(256), 0, stream, params); break; \
      case 2 + tsm_host::kYuvYv12: TSM_KLAUNCH(KERNEL<Yv12>, dim3(grid_), dim3(256), 0, stream, params); break; \
      case 2 + tsm_host::kYuvP010: TSM_KLAUNCH(KERNEL<P010>, dim3(grid_), dim3(256), 0, stream, params); break; \
      case 2 + tsm_host::kYuvYuyv: TSM_KLAUNCH(KERNEL<Yuyv>, dim3(grid_), dim3(256), 0, stream, params); break; \
      case 2 + tsm_host::kYuvUyvy: TSM_KLAUNCH(KERNEL<Uyvy>, dim3(grid_), dim3(256), 0, stream, params); break; \
      default:                                                                                              \
        if (is_u8)                                                                                          \
          TSM_KLAUNCH(KERNEL<unsigned char>, dim3(grid_), dim3(256), 0, stream, params);                    \
        else                                                                                                \
          TSM_KLAUNCH(KERNEL<float>, dim3(grid_), dim3(256), 0, stream, params);                            \
    }                                                                                                       \
  } while (0)

hipError_t launch_preprocess(const PreprocParams &p, hipStream_t s) {
  if (p.n <= 0 || !crop_window_ok(p) || !yuv_frames_ok(p.src_yuv, p.src, p.h, p.w)) return hipErrorInvalidValue;
  TSM_LAUNCH_ROWS(preprocess_kernel, p.src_is_u8, p.src_yuv, p.n, p.crop, p.out_mode, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// gather_clips: the clip iterator of the dataset loop (utils/inference_count.py:411-414, video[i:i + 16:2] with a
// zero-padded tail) over TRANSFORMED frames that sit in a device buffer: out[c][k] = frame of source index
// step * (first_clip + c) + stride * k, the buffer's pad frame where that index is past the video's end.  Frames are
// opaque rows of frame_bytes (any packed layout); 16-byte copies, four in flight per thread.  HBM-bound and tiny
// next to the forward (a batch of 32 clips moves 2 x 205 MB: 0.1 ms) -- it exists so that the loop's only device work
// between two forwards is this library's: torch's index_select costs two first-use code-object loads (4 + 150 ms with
// the GPU idle at the head of every cold dataset job, profiles/r03_config4_gpu_gaps_pieces.txt).
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) gather_clips_kernel(const GatherParams p) {
  const int64_t row = p.row0 + blockIdx.y;          // (clip, segment) of the output
  const int64_t c = row / p.n_segment;
  const int k = (int)(row - c * p.n_segment);
  const int64_t src_frame = (int64_t)p.clip_step * (p.first_clip + c) + (int64_t)p.clip_stride * k;
  const int64_t j = src_frame < p.total_frames ? src_frame / p.clip_stride - p.first_frame : p.pad_frame;
  const uint4 *src = reinterpret_cast<const uint4 *>(static_cast<const char *>(p.frames) + j * p.frame_bytes);
  uint4 *dst = reinterpret_cast<uint4 *>(static_cast<char *>(p.out) + row * p.frame_bytes);
  const int64_t n16 = p.frame_bytes / 16;
  for (int64_t i = (int64_t)blockIdx.x * 1024 + threadIdx.x; i < n16; i += (int64_t)gridDim.x * 1024) {
    uint4 v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * 256 < n16) v[u] = src[i + u * 256];
#pragma unroll
    for (int u = 0; u < 4; ++u)
      if (i + u * 256 < n16) dst[i + u * 256] = v[u];
  }
}

hipError_t launch_gather_clips(const GatherParams &p_in, hipStream_t s) {
  GatherParams p = p_in;
  // every index the kernel will form, checked here: a clip starts inside its video, the first and the last in-video position of
  // the range lie in the buffer, and the pad frame
  tsm_host::WindowRange r;
  if (!p.frames || !p.out || p.frame_bytes <= 0 || p.frame_bytes % 16 != 0 ||
      !tsm_host::clip_window_range(p.total_frames, p.first_clip, p.n_clips, p.n_segment, p.clip_step, p.clip_stride, p.first_frame,
                                   p.n_frames, &r))
    return hipErrorInvalidValue;
  // a padded tail reads the pad frame: it must lie in the buffer and must not be one of the range's own video frames (a
  // mis-sized buffer or a wrong first_frame / total_frames pair would otherwise pass a real frame off as the zero frame)
  if (r.tail && (p.pad_frame < 0 || p.pad_frame >= p.n_frames || (p.pad_frame >= r.first && p.pad_frame <= r.last)))
    return hipErrorInvalidValue;
  const int64_t n16 = p.frame_bytes / 16;
  const unsigned gx = (unsigned)((n16 + 1023) / 1024 < 64 ? (n16 + 1023) / 1024 : 64);
  // grid.y holds at most 65535 (clip, segment) rows: longer ranges are cut into several launches here, so that the limit
  // is not a property of the C ABI
  const int64_t rows = (int64_t)p.n_clips * p.n_segment;
  for (int64_t r0 = 0; r0 < rows; r0 += 65535) {
    p.row0 = r0;
    const int64_t ny = rows - r0 < 65535 ? rows - r0 : 65535;
    TSM_KLAUNCH(gather_clips_kernel, dim3(gx, (unsigned)ny), dim3(256), 0, s, p);
    const hipError_t st = hipGetLastError();
    if (st != hipSuccess) return st;
  }
  return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// preprocess_clips: the person-crop test transform (datasets/build.py:123-129 of the reference: PersonCrop ->
// Resize((size, size)) -> Normalize, from the detector's box on) fused with the clip iterator above, one launch from the
// staged RAW frames to the engine's packed input: out[c][k] = source frame clip_step * (first_clip + c) + clip_stride * k,
// cropped to clip c's box (top, left, bh, bw), resized to size x size, normalised.  The transform sits BEHIND the gather
// because the box is per clip: an even frame shared by two overlapping windows is cropped twice, with two boxes.
//   * zero fill: a tap of the box outside the frame has the value 0 and is not read (torchvision's tensor crop pads with
//     zeros BEFORE Normalize: a pixel wholly outside becomes (0 - mean) / std);
//   * no person: bh <= 0 or bw <= 0 stands for the whole frame (0, 0, h, w) (transform.py:254 `if w * h == 0: return images`);
//   * padded tail: a source index >= total_frames is the reference's zero frame: every channel (0 - mean) / std, nothing is
//     read and the buffer needs no pad frame.
// The sampler (box_pixel) is preprocess_pixel's arithmetic in box coordinates.
// TOTAL in the boxes: they live in device memory, so no host check can see them; for ANY int32 contents the kernel reads only
// inside the frames it was given -- the box index is clamped to the box, the sum with top / left is formed in 64 bits and a
// tap is read only where 0 <= y < h and 0 <= x < w.  (The frame index is the host's to validate: launch_preprocess_clips.)
// ---------------------------------------------------------------------------------------------
// The sampler of the box sources (ClipRows, WindowRows in person-crop mode): preprocess_pixel in the coordinates of a box
// (top, left, bh, bw; bh, bw > 0) of an h x w frame resized to size x size, total in the box.
template <typename T>
__device__ __forceinline__ void box_pixel(const Taps<T> &frame, int h, int w, int64_t top, int64_t left, int bh, int bw, int size,
                                          float pre_scale, int oy, int ox, float *v) {
#pragma clang fp contract(off)
  const float fy = sample_coord((float)bh / (float)size, (float)oy);
  const float fx = sample_coord((float)bw / (float)size, (float)ox);
  // (int) of a float at or above 2^31 is undefined: sides near INT32_MAX are held below it, and the index inside the box
  const float big = 2147483520.f;
  int y0 = (int)(fy < big ? fy : big), x0 = (int)(fx < big ? fx : big);
  y0 = y0 < bh - 1 ? y0 : bh - 1;
  x0 = x0 < bw - 1 ? x0 : bw - 1;
  const int y1 = y0 + (y0 < bh - 1 ? 1 : 0), x1 = x0 + (x0 < bw - 1 ? 1 : 0);
  const float h1 = fy - (float)y0, h0 = 1.f - h1, w1 = fx - (float)x0, w0 = 1.f - w1;
  // image coordinates of the four taps, in 64 bits (top + y0 leaves int32 for a hostile box); a tap outside the frame is 0
  const int64_t iy0 = top + y0, iy1 = top + y1, ix0 = left + x0, ix1 = left + x1;
  const bool vy0 = iy0 >= 0 && iy0 < h, vy1 = iy1 >= 0 && iy1 < h;
  const bool vx0 = ix0 >= 0 && ix0 < w, vx1 = ix1 >= 0 && ix1 < w;
  // (addresses are formed from coordinates held inside the frame: no product of a hostile sum, no pointer outside the buffer)
  float t[4][3];
  frame.quad(vy0 ? iy0 : 0, vy1 ? iy1 : 0, vx0 ? ix0 : 0, vx1 ? ix1 : 0, vy0 && vx0, vy0 && vx1, vy1 && vx0, vy1 && vx1, t);
#pragma unroll
  for (int c = 0; c < 3; ++c) v[c] = bilinear_normalised(t[0][c], t[1][c], t[2][c], t[3][c], w0, w1, h0, h1, pre_scale, c);
}

template <typename T>
struct ClipRows {
  const ClipPreprocParams &p;
  struct Row {
    Taps<T> frame;
    int64_t top, left;
    int bh, bw;
  };
  __device__ __forceinline__ bool locate(int64_t f, Row *r) const {
    const int64_t c = f / p.n_segment;             // f = the (clip, segment) row of the output
    const int k = (int)(f - c * p.n_segment);
    const int64_t s = (int64_t)p.clip_step * (p.first_clip + c) + (int64_t)p.clip_stride * k;
    if (s >= p.total_frames) return false;
    // the clip's box: four dwords, the same for every thread of (nearly every) wave -- ONE 16-byte load (two dependent 8-byte
    // loads are one more memory latency per group), which asks no alignment of the caller
    typedef int box_t __attribute__((ext_vector_type(4), aligned(4)));
    const box_t b = *reinterpret_cast<const box_t *>(p.boxes + c * 4);
    const bool person = b[2] > 0 && b[3] > 0;
    r->top = person ? b[0] : 0;
    r->left = person ? b[1] : 0;
    r->bh = person ? b[2] : p.h;
    r->bw = person ? b[3] : p.w;
    r->frame = Taps<T>::of(p.src, s / p.clip_stride - p.first_frame, p.h, p.w, p.nv12);
    return true;
  }
  __device__ __forceinline__ void pixel(const Row &r, int oy, int ox, float *v) const {
    box_pixel<T>(r.frame, p.h, p.w, r.top, r.left, r.bh, r.bw, p.size, p.pre_scale, oy, ox, v);
  }
};

template <typename T>
__global__ void __launch_bounds__(256) preprocess_clips_kernel(const ClipPreprocParams p) {
  preprocess_rows(p.dst, p.out_mode, p.size, (int64_t)p.n_clips * p.n_segment, ClipRows<T>{p});
}

hipError_t launch_preprocess_clips(const ClipPreprocParams &p, hipStream_t s) {
  // every frame index the kernel will form, checked here (launch_gather_clips' rules; there is no pad frame to check)
  tsm_host::WindowRange r;
  if (!p.src || !p.dst || !p.boxes || p.h <= 0 || p.w <= 0 || p.size <= 0 || p.out_mode < 0 || p.out_mode > 3 ||
      !yuv_frames_ok(p.src_yuv, p.src, p.h, p.w) ||
      !tsm_host::clip_window_range(p.total_frames, p.first_clip, p.n_clips, p.n_segment, p.clip_step, p.clip_stride, p.first_frame,
                                   p.n_frames, &r))
    return hipErrorInvalidValue;
  TSM_LAUNCH_ROWS(preprocess_clips_kernel, p.src_is_u8, p.src_yuv, (int64_t)p.n_clips * p.n_segment, p.size, p.out_mode, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// preprocess_indexed: the centre-crop test transform (preprocess_kernel: build_test_transform(person_crop=False)) through a
// DEVICE index table, one launch from the staged RAW frames to the engine's packed input: out row r = the transform of
// buffer frame index[r].  This is the access pattern of the reference's FrameDataset (datasets/common.py:99-117:
// sample_frames(total, 8, start, random=False) per labelled segment): irregular lists -- a segment shorter than 8 frames
// repeats frames, two segments of one video share no window, unsampled frames are never needed -- that the regular windows
// of gather_clips / preprocess_clips (step * c + stride * k) cannot express.  A frame two rows share is transformed twice:
// the rows are independent, and the alternative (transform each staged frame once, then gather) is a second pass and a
// transformed intermediate in memory.
// The pixel is preprocess_pixel's, so a row equals preprocess_kernel's row for the same frame bit for bit.
// TOTAL in the table: it lives in device memory, so no host check can see it; for ANY int32 contents the kernel reads only
// inside the frames it was given -- the entry is range-tested first, and only then widened to 64 bits and multiplied into a
// frame address.  An entry outside [0, n_frames) reads nothing and yields the normalised zero frame (0 - mean) / std, as
// preprocess_clips' padded tail does.  The table entry is one dword, the same for (nearly) every thread of a wave.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct IndexedRows {
  const IndexedPreprocParams &q;
  using Row = Taps<T>;
  __device__ __forceinline__ bool locate(int64_t f, Row *frame) const {
    const int j = q.index[f];
    if (j < 0 || (int64_t)j >= q.n_frames) return false;
    *frame = Taps<T>::of(q.pp.src, j, q.pp.h, q.pp.w, q.pp.nv12);
    return true;
  }
  __device__ __forceinline__ void pixel(const Row &frame, int oy, int ox, float *v) const { preprocess_pixel<T>(q.pp, frame, oy, ox, v); }
};

template <typename T>
__global__ void __launch_bounds__(256) preprocess_indexed_kernel(const IndexedPreprocParams q) {
  preprocess_rows(q.pp.dst, q.pp.out_mode, q.pp.crop, q.n_rows, IndexedRows<T>{q});
}

hipError_t launch_preprocess_indexed(const IndexedPreprocParams &q, hipStream_t s) {
  const PreprocParams &p = q.pp;
  if (!p.src || !p.dst || !q.index || q.n_frames <= 0 || q.n_rows <= 0 || !crop_window_ok(p) || p.out_mode < 0 || p.out_mode > 3 ||
      !yuv_frames_ok(p.src_yuv, p.src, p.h, p.w))
    return hipErrorInvalidValue;
  TSM_LAUNCH_ROWS(preprocess_indexed_kernel, p.src_is_u8, p.src_yuv, q.n_rows, p.crop, p.out_mode, s, q);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// preprocess_windows: either test transform over windows of DIFFERENT frame sizes, one launch from raw frames to the engine's
// packed input in batch order -- a step of StreamBatcher, whose streams (phones, webcams, uploaded clips) differ in
// resolution.  Output row f is frame f % n_segment of window f / n_segment; the window's 8-dword descriptor {off_lo, off_hi,
// h, w, top, left, bh, bw} says where its n_segment contiguous frames [h, w, 3] start in the arena (a byte offset) and, in
// person-crop mode, its box.  The descriptor is the same for (nearly) every thread of a wave: two 16-byte loads.
//   * person_crop 0: Resize(resize) + CenterCrop(crop) with the geometry of THIS window's size, computed here in integers
//     (tsm_host::center_crop_geometry_int = the host's center_crop_geometry), the pixel preprocess_pixel's: a row equals
//     preprocess_kernel's row for the same frame bit for bit.  The box words are ignored.
//   * person_crop 1: the box -> Resize((crop, crop)) by box_pixel, preprocess_clips' rules (zero fill, bh <= 0 or bw <= 0 =
//     the whole frame): a row equals preprocess_clips_kernel's row for the same frame and box bit for bit.
// TOTAL in the table: it lives in device memory, so no host check can see it.  tsm_host::window_descriptor_ok decides, in
// int64 without overflow for ANY int32 words, whether the window lies in the arena (and, mode 0, whether the crop fits the
// resized frame) BEFORE an address is formed; every row of a window that fails is the normalised zero frame and reads nothing.
// ---------------------------------------------------------------------------------------------
template <typename T>
struct WindowRows {
  const WindowPreprocParams &p;
  struct Row {
    Taps<T> frame;
    int h, w;
    int top, left;      // mode 0: the crop window's corner in the resized frame; mode 1: the box's corner in the source frame
    int sh, sw;         // mode 0: the resized size (nh, nw); mode 1: the box's size (bh, bw)
  };
  __device__ __forceinline__ bool locate(int64_t f, Row *r) const {
    const int64_t c = f / p.n_segment;
    const int k = (int)(f - c * p.n_segment);
    typedef int desc_t __attribute__((ext_vector_type(4)));         // (16-byte aligned: the launcher checks the table's base)
    const desc_t *dp = reinterpret_cast<const desc_t *>(p.desc) + c * 2;
    const desc_t lo = dp[0], hi = dp[1];
    const int32_t d[tsm_host::kWindowDescWords] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    int64_t off;
    tsm_host::CropGeometry g;
    if (!Taps<T>::descriptor_ok(d, p.n_segment, p.arena_bytes, !p.person_crop, p.resize, p.crop, &off, &g)) return false;
    r->h = d[2];
    r->w = d[3];
    r->frame = Taps<T>::of(static_cast<const char *>(p.arena) + off, k, r->h, r->w, p.nv12);
    if (p.person_crop) {
      const bool person = d[6] > 0 && d[7] > 0;
      r->top = person ? d[4] : 0;
      r->left = person ? d[5] : 0;
      r->sh = person ? d[6] : r->h;
      r->sw = person ? d[7] : r->w;
    } else {
      r->top = g.top;
      r->left = g.left;
      r->sh = g.nh;
      r->sw = g.nw;
    }
    return true;
  }
  __device__ __forceinline__ void pixel(const Row &r, int oy, int ox, float *v) const {
    if (p.person_crop) {
      box_pixel<T>(r.frame, r.h, r.w, r.top, r.left, r.sh, r.sw, p.crop, p.pre_scale, oy, ox, v);
    } else {
      PreprocParams q;            // (preprocess_pixel reads only these)
      q.h = r.h; q.w = r.w; q.nh = r.sh; q.nw = r.sw; q.top = r.top; q.left = r.left; q.pre_scale = p.pre_scale;
      preprocess_pixel<T>(q, r.frame, oy, ox, v);
    }
  }
};

template <typename T>
__global__ void __launch_bounds__(256) preprocess_windows_kernel(const WindowPreprocParams p) {
  preprocess_rows(p.dst, p.out_mode, p.crop, (int64_t)p.n_windows * p.n_segment, WindowRows<T>{p});
}

hipError_t launch_preprocess_windows(const WindowPreprocParams &p, hipStream_t s) {
  if (!p.arena || !p.dst || !p.desc || (reinterpret_cast<uintptr_t>(p.arena) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.desc) & 15) != 0 ||
      p.arena_bytes <= 0 || p.n_windows <= 0 || p.n_segment <= 0 || p.resize <= 0 || p.crop <= 0 || p.out_mode < 0 || p.out_mode > 3 ||
      (p.person_crop != 0 && p.person_crop != 1) || (!p.person_crop && p.crop > p.resize))
    return hipErrorInvalidValue;
  TSM_LAUNCH_ROWS(preprocess_windows_kernel, p.src_is_u8, p.src_yuv, (int64_t)p.n_windows * p.n_segment, p.crop, p.out_mode, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// maxpool 3x3 stride 2 pad 1, NHWC; one thread per (output pixel, channel group).
// ---------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(256) maxpool3x3s2_kernel(const float *__restrict__ x,
                                                           float *__restrict__ y, int n, int hi, int wi,
                                                           int ho, int wo, int cg) {
  constexpr int GF = Fmt<FMT>::gf;
  const int64_t total = (int64_t)n * ho * wo * cg;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int g = (int)(i % cg);
    int64_t pix = i / cg;
    const int ox = (int)(pix % wo);
    pix /= wo;
    const int oy = (int)(pix % ho);
    const int64_t f = pix / ho;
    float m[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = -INFINITY;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
      const int iy = oy * 2 - 1 + ky;
      if ((unsigned)iy >= (unsigned)hi) continue;
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const int ix = ox * 2 - 1 + kx;
        if ((unsigned)ix >= (unsigned)wi) continue;
        float v[8];
        load_group<FMT>(x + (((f * hi + iy) * wi + ix) * cg + g) * GF, v);
#pragma unroll
        for (int e = 0; e < 8; ++e) m[e] = fmaxf(m[e], v[e]);
      }
    }
    store_group<FMT>(y + i * GF, m);
  }
}

hipError_t launch_maxpool3x3s2(const float *x, float *y, int n, int hi, int wi, int c, int prec, hipStream_t s) {
  const int gch = prec == kPrecF32 ? 4 : 8;
  if (c % gch != 0) return hipErrorInvalidValue;
  const int ho = (hi + 2 - 3) / 2 + 1, wo = (wi + 2 - 3) / 2 + 1;
  const int cg = c / gch;
  const int64_t total = (int64_t)n * ho * wo * cg;
  TSM_DISPATCH_FMT(prec, maxpool3x3s2_kernel, grid_for(total, 8192), s, x, y, n, hi, wi, ho, wo, cg);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Temporal max-pool (TemporalPool in front of layer2: max_pool3d, kernel (3,1,1), stride (2,1,1), padding (1,0,0)) on NHWC
// tensors in the storage format: output frame t' of a clip = max over its frames {2t'-1, 2t', 2t'+1} cut to [0, T), T even.
// One thread owns a (clip, pixel, channel group) column and walks its T frames in order, keeping the last odd frame in
// registers: every input group is loaded once, every output group stored once.  No LDS, no atomics; nothing depends on the
// grid or on the other clips.  A group's words stay as they are: fp32 values by fmaxf; split-bf16 pairs (hi, lo) compared by
// hi, then by lo -- |lo| <= ulp(hi) / 2, so that is the order of hi + lo -- and the winner's pair copied.  fp32 and split-bf16
// only (the launcher refuses bf16: no bf16 engine pools).
// ---------------------------------------------------------------------------------------------
template <int FMT>
struct PoolGroup {
  u32x4 h, l;   // fp32: h = the four floats' bits; split-bf16: h | l, 8 elements each
};

template <int FMT>
__device__ __forceinline__ PoolGroup<FMT> pool_load(const float *p) {
  PoolGroup<FMT> g;
  g.h = *reinterpret_cast<const u32x4 *>(p);
  g.l = FMT == kPrecBf16x3 ? *reinterpret_cast<const u32x4 *>(p + 4) : u32x4{0u, 0u, 0u, 0u};
  return g;
}

template <int FMT>
__device__ __forceinline__ void pool_store(float *p, const PoolGroup<FMT> &g) {
  *reinterpret_cast<u32x4 *>(p) = g.h;
  if (FMT == kPrecBf16x3) *reinterpret_cast<u32x4 *>(p + 4) = g.l;
}

template <int FMT>
__device__ __forceinline__ PoolGroup<FMT> pool_max(const PoolGroup<FMT> &a, const PoolGroup<FMT> &b) {
  PoolGroup<FMT> m;
  m.l = u32x4{0u, 0u, 0u, 0u};
  if (FMT == kPrecF32) {   // (whole vectors through the cast: element by element on the words)
    const f32x4 fa = __builtin_bit_cast(f32x4, a.h), fb = __builtin_bit_cast(f32x4, b.h);
    m.h = __builtin_bit_cast(u32x4, f32x4{fmaxf(fa[0], fb[0]), fmaxf(fa[1], fb[1]), fmaxf(fa[2], fb[2]), fmaxf(fa[3], fb[3])});
    return m;
  }
#pragma unroll
  for (int w = 0; w < 4; ++w) {
    {
      unsigned keep_a = 0u;   // the 16-bit halves of word w that a wins
#pragma unroll
      for (int half = 0; half < 2; ++half) {
        const int e = 2 * w + half;
        const float ah = split_elem(a.h, e), bh = split_elem(b.h, e);
        bool a_wins = ah > bh;
        if (FMT == kPrecBf16x3) a_wins = a_wins || (ah == bh && split_elem(a.l, e) > split_elem(b.l, e));
        if (a_wins) keep_a |= half ? 0xFFFF0000u : 0x0000FFFFu;
      }
      m.h[w] = (a.h[w] & keep_a) | (b.h[w] & ~keep_a);
      if (FMT == kPrecBf16x3) m.l[w] = (a.l[w] & keep_a) | (b.l[w] & ~keep_a);
    }
  }
  return m;
}

template <int FMT>
__global__ void __launch_bounds__(256) temporal_maxpool_kernel(const float *__restrict__ x, float *__restrict__ y,
                                                               int64_t n_clips, int T, int64_t frame_groups) {
  constexpr int GF = Fmt<FMT>::gf;
  const int64_t total = n_clips * frame_groups;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t frame = frame_groups * GF;   // floats per frame
  const int t_out = T / 2;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int64_t clip = i / frame_groups, col = i - clip * frame_groups;
    const float *src = x + clip * T * frame + col * GF;
    float *dst = y + clip * t_out * frame + col * GF;
    PoolGroup<FMT> odd = pool_load<FMT>(src);   // (frame 0 stands in for frame -1: max(x0, x0, x1) = max(x0, x1))
    for (int t = 0; t < t_out; ++t) {
      const PoolGroup<FMT> even = t == 0 ? odd : pool_load<FMT>(src + (int64_t)(2 * t) * frame);
      const PoolGroup<FMT> next = pool_load<FMT>(src + (int64_t)(2 * t + 1) * frame);
      pool_store<FMT>(dst + (int64_t)t * frame, pool_max<FMT>(pool_max<FMT>(odd, even), next));
      odd = next;
    }
  }
}

hipError_t launch_temporal_maxpool(const float *x, float *y, int64_t n_clips, int T, int64_t hw, int c, int prec, hipStream_t s) {
  const int gch = prec == kPrecF32 ? 4 : 8;
  if (n_clips <= 0 || hw <= 0 || c <= 0 || c % gch != 0 || tsm_host::temporal_pool_segments(T) < 0) return hipErrorInvalidValue;
  if (prec != kPrecF32 && prec != kPrecBf16x3) return hipErrorInvalidValue;   // (no bf16 engine pools: tsm_set_temporal_pool)
  const int64_t frame_groups = hw * (c / gch);
  const unsigned grid = grid_for(n_clips * frame_groups, 8192);
  if (prec == kPrecF32)
    TSM_KLAUNCH(temporal_maxpool_kernel<kPrecF32>, dim3(grid), dim3(256), 0, s, x, y, n_clips, T, frame_groups);
  else
    TSM_KLAUNCH(temporal_maxpool_kernel<kPrecBf16x3>, dim3(grid), dim3(256), 0, s, x, y, n_clips, T, frame_groups);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Stand-alone temporal shift (NHWC fp32). One thread per 16-B channel quad; fold % 4 == 0 so a quad
// never straddles a fold boundary.  tsm.py:35-50.  (The forward uses the conv kernel's fused loader.)
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) temporal_shift_kernel(const float *__restrict__ x,
                                                             float *__restrict__ y, int64_t n_frames,
                                                             int n_segment, int64_t hw, int c4, int fold4) {
  const int64_t total = n_frames * hw * c4;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const int64_t frame_quads = hw * c4;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
    const int cq = (int)(i % c4);
    const int64_t f = i / frame_quads;
    const int t = (int)(f % n_segment);
    int dt = cq < fold4 ? 1 : (cq < 2 * fold4 ? -1 : 0);
    const bool ok = dt == 1 ? t < n_segment - 1 : (dt == -1 ? t > 0 : true);
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (ok) v = *reinterpret_cast<const f32x4 *>(x + (i + dt * frame_quads) * 4);
    *reinterpret_cast<f32x4 *>(y + i * 4) = v;
  }
}

hipError_t launch_temporal_shift(const float *x, float *y, int64_t n_frames, int n_segment, int64_t hw,
                                 int c, int fold, hipStream_t s) {
  if (c % 4 != 0 || fold % 4 != 0 || n_segment <= 0 || n_frames % n_segment != 0) return hipErrorInvalidValue;
  const int64_t total = n_frames * hw * (c / 4);
  TSM_KLAUNCH(temporal_shift_kernel, dim3(grid_for(total, 8192)), dim3(256), 0, s, x, y, n_frames,
                     n_segment, hw, c / 4, fold / 4);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Head.  logits[b] = fc( mean_t mean_hw feat[b,t,hw,:] ) + bias  (avg-pool, FC and the segment mean
// are all linear, so pooling first is exact up to fp32 summation order).  tsm.py:411-419.
//   head_pool: grid (n_frames, ...): per-frame average pool into pooled[n_frames, c] (fp32);
//              one thread per channel group, rows streamed with 16-byte loads.
//   head_fc  : grid (n_clips, num_class) x 64 lanes: mean over the clip's frames, dot with one class row.
// ---------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(256) head_pool_kernel(const float *__restrict__ feat,
                                                        float *__restrict__ pooled, int rows, int c) {
  constexpr int GF = Fmt<FMT>::gf, GC = Fmt<FMT>::ch;
  const int b = blockIdx.x;
  const int t = blockIdx.y * 256 + threadIdx.x;
  const int cg = c / GC;
  if (t >= cg) return;
  const float *src = feat + ((size_t)b * rows * cg + t) * GF;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  // rows are added in order; unrolled by 7 (49 = 7 x 7 at 224^2) so that the loads of a group are in flight together
#pragma unroll 7
  for (int r = 0; r < rows; ++r) {
    float v[8];
    load_group<FMT>(src + (size_t)r * cg * GF, v);
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[e] += v[e];
  }
#pragma unroll
  for (int e = 0; e < GC; ++e) pooled[(size_t)b * c + t * GC + e] = acc[e] / (float)rows;
}

// one 64-lane workgroup per (clip, class): every lane streams its share of the 2048 channels over the
// clip's T pooled frames (independent loads), then a wave reduction
__global__ void __launch_bounds__(64) head_fc_kernel(const float *__restrict__ pooled,
                                                     const float *__restrict__ fc_w,
                                                     const float *__restrict__ fc_b,
                                                     float *__restrict__ logits, int c, int num_class,
                                                     int n_segment) {
  const int b = blockIdx.x, cls = blockIdx.y;
  const int lane = threadIdx.x;
  const float *pv = pooled + (size_t)b * n_segment * c;  // per-frame pooled features of this clip
  const float *wv = fc_w + (size_t)cls * c;
  float s = 0.f;
  for (int k = lane * 4; k < c; k += 256) {
    f32x4 f = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 8
    for (int t = 0; t < n_segment; ++t) f += *reinterpret_cast<const f32x4 *>(pv + (size_t)t * c + k);
    const f32x4 w = *reinterpret_cast<const f32x4 *>(wv + k);
    s += (f[0] * w[0] + f[1] * w[1]) + (f[2] * w[2] + f[3] * w[3]);
  }
  s /= (float)n_segment;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
  if (lane == 0) logits[(size_t)b * num_class + cls] = s + fc_b[cls];
}

hipError_t launch_head(const float *feat, const float *fc_w, const float *fc_b, float *pooled,
                       float *logits, int n_clips, int n_segment, int hw, int c, int num_class, int prec,
                       hipStream_t s) {
  if (n_clips <= 0 || c <= 0 || c % 8 != 0) return hipErrorInvalidValue;
  const int cg = c / (prec == kPrecF32 ? 4 : 8);
  const dim3 grid(n_clips * n_segment, (cg + 255) / 256);
  if (prec == kPrecBf16x3)
    TSM_KLAUNCH(head_pool_kernel<kPrecBf16x3>, grid, dim3(256), 0, s, feat, pooled, hw, c);
  else if (prec == kPrecBf16)
    TSM_KLAUNCH(head_pool_kernel<kPrecBf16>, grid, dim3(256), 0, s, feat, pooled, hw, c);
  else
    TSM_KLAUNCH(head_pool_kernel<kPrecF32>, grid, dim3(256), 0, s, feat, pooled, hw, c);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  TSM_KLAUNCH(head_fc_kernel, dim3(n_clips, num_class), dim3(64), 0, s, pooled, fc_w, fc_b, logits, c,
                     num_class, n_segment);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Per-segment head (consensus_type='identity', tsm.py:165-174): logits[f] = fc( mean_hw feat[f,hw,:] ) + bias for every
// FRAME, no mean over the segments -- so nothing crosses a frame and the whole head is ONE launch, one 256-thread workgroup
// per frame, and `pooled` never goes to memory:
//   phase 1: head_pool_kernel's loop (same row order, same division: the pooled value of a frame is the avg head's to the
//            bit), one channel group per thread and pass, into LDS as fp32 (c <= 2048: 8 KB);
//   phase 2: the four waves take the classes round robin; the lanes stride the channels with 16-byte LDS reads and fc_w
//            loads (head_fc_kernel's k order and pairing), a wave reduction, lane 0 stores.
// ---------------------------------------------------------------------------------------------
constexpr int kHeadSegMaxC = 2048;

template <int FMT>
__global__ void __launch_bounds__(256) head_seg_kernel(const float *__restrict__ feat, const float *__restrict__ fc_w,
                                                       const float *__restrict__ fc_b, float *__restrict__ logits,
                                                       int rows, int c, int num_class) {
  constexpr int GF = Fmt<FMT>::gf, GC = Fmt<FMT>::ch;
  __shared__ __attribute__((aligned(16))) float pooled[kHeadSegMaxC];
  const int b = blockIdx.x;
  const int cg = c / GC;
  for (int t = threadIdx.x; t < cg; t += 256) {
    const float *src = feat + ((size_t)b * rows * cg + t) * GF;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 7
    for (int r = 0; r < rows; ++r) {
      float v[8];
      load_group<FMT>(src + (size_t)r * cg * GF, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < GC; ++e) pooled[t * GC + e] = acc[e] / (float)rows;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  for (int cls = wave; cls < num_class; cls += 4) {
    const float *wv = fc_w + (size_t)cls * c;
    float s = 0.f;
    for (int k = lane * 4; k < c; k += 256) {
      const f32x4 f = *reinterpret_cast<const f32x4 *>(pooled + k);
      const f32x4 w = *reinterpret_cast<const f32x4 *>(wv + k);
      s += (f[0] * w[0] + f[1] * w[1]) + (f[2] * w[2] + f[3] * w[3]);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_down(s, off, 64);
    if (lane == 0) logits[(size_t)b * num_class + cls] = s + fc_b[cls];
  }
}

hipError_t launch_head_segments(const float *feat, const float *fc_w, const float *fc_b, float *logits, int n_frames,
                                int hw, int c, int num_class, int prec, hipStream_t s) {
  if (n_frames <= 0 || hw <= 0 || num_class <= 0 || c <= 0 || c % 8 != 0 || c > kHeadSegMaxC) return hipErrorInvalidValue;
  TSM_DISPATCH_FMT(prec, head_seg_kernel, n_frames, s, feat, fc_w, fc_b, logits, hw, c, num_class);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Frame embeddings (utils/common.py:79-116, cnn_feature / video_feature: a ResNet with num_classes=0 yields the pooled
// vector of every frame): pooled[f] = mean_hw feat[f,hw,:] and unit[f] = pooled[f] / ||pooled[f]||2, the row scikit-learn's
// pairwise_distances(metric='cosine') normalises to (utils/common.py:133).  ONE launch, one 256-thread workgroup per frame,
// no scratch buffer; either output may be null:
//   phase 1: head_seg_kernel's phase 1 (same row order, same division: a frame's pooled value is head_pool_kernel's to the
//            bit) into LDS;
//   phase 2: sum of squares in an order that depends on c alone -- thread t adds channels 4t .. 4t + 3, then 1024 + 4t ..,
//            ascending; a shuffle tree per wave; ((w0 + w1) + (w2 + w3)) over the four waves -- so a frame's unit row does
//            not depend on n_frames or on which frames share the launch;
//   phase 3: norm = sqrtf(ss), 0 replaced by 1 (sklearn.preprocessing.normalize: an all-zero row stays all-zero), unit = pooled / norm.
// ---------------------------------------------------------------------------------------------
template <int FMT>
__global__ void __launch_bounds__(256) pool_feat_kernel(const float *__restrict__ feat, float *__restrict__ pooled_out,
                                                        float *__restrict__ unit_out, int rows, int c) {
  constexpr int GF = Fmt<FMT>::gf, GC = Fmt<FMT>::ch;
  __shared__ __attribute__((aligned(16))) float pooled[kHeadSegMaxC];
  __shared__ float wave_ss[4];
  const int b = blockIdx.x;
  const int cg = c / GC;
  for (int t = threadIdx.x; t < cg; t += 256) {
    const float *src = feat + ((size_t)b * rows * cg + t) * GF;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 7
    for (int r = 0; r < rows; ++r) {
      float v[8];
      load_group<FMT>(src + (size_t)r * cg * GF, v);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc[e] += v[e];
    }
#pragma unroll
    for (int e = 0; e < GC; ++e) pooled[t * GC + e] = acc[e] / (float)rows;
  }
  __syncthreads();
  float ss = 0.f;
  for (int k = threadIdx.x * 4; k < c; k += 1024) {
    const f32x4 f = *reinterpret_cast<const f32x4 *>(pooled + k);
    if (pooled_out) *reinterpret_cast<f32x4 *>(pooled_out + (size_t)b * c + k) = f;
#pragma unroll
    for (int e = 0; e < 4; ++e) ss += f[e] * f[e];
  }
  if (!unit_out) return;   // (uniform over the workgroup)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) ss += __shfl_xor(ss, off, 64);
  if ((threadIdx.x & 63) == 0) wave_ss[threadIdx.x >> 6] = ss;
  __syncthreads();
  float norm = sqrtf((wave_ss[0] + wave_ss[1]) + (wave_ss[2] + wave_ss[3]));
  if (norm == 0.f) norm = 1.f;
  for (int k = threadIdx.x * 4; k < c; k += 1024) {
    const f32x4 f = *reinterpret_cast<const f32x4 *>(pooled + k);
    *reinterpret_cast<f32x4 *>(unit_out + (size_t)b * c + k) = f32x4{f[0] / norm, f[1] / norm, f[2] / norm, f[3] / norm};
  }
}

hipError_t launch_pool_features(const float *feat, float *pooled, float *unit, int n_frames, int hw, int c, int prec,
                                hipStream_t s) {
  if (n_frames <= 0 || hw <= 0 || c <= 0 || c % 8 != 0 || c > kHeadSegMaxC || (!pooled && !unit)) return hipErrorInvalidValue;
  TSM_DISPATCH_FMT(prec, pool_feat_kernel, n_frames, s, feat, pooled, unit, hw, c);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// K9: logits -> per-clip state on the GPU (utils/eval.py:153-164 + to_softmax, utils/visualize.py:140-150):
// optional fp32 softmax over the classes, FIRST maximum, class id if its score >= threshold else -1.  One thread per
// clip (n_clips x num_class is tiny; the point is that a streaming step copies 8 bytes per window to the host instead
// of the logits, and needs no host-side numpy pass).  The sum runs in numpy's order for rows of 8..128 elements
// (8 strided partial sums, a fixed tree, then the remainder), so probabilities match the host path up to the 1-ulp
// freedom of expf itself.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64) scores_to_states_kernel(const float *__restrict__ logits, int n, int c, int softmax,
                                                              float threshold, int *__restrict__ states,
                                                              float *__restrict__ top) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const float *s = logits + (size_t)i * c;
  float best = 0.f;
  int arg = 0;
  if (softmax) {
    float mx = s[0];
    for (int j = 1; j < c; ++j) mx = fmaxf(mx, s[j]);
    float sum;
    if (c >= 8 && c <= 128) {
      float r[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) r[j] = expf(s[j] - mx);
      int j = 8;
      for (; j + 8 <= c; j += 8)
#pragma unroll
        for (int q = 0; q < 8; ++q) r[q] += expf(s[j + q] - mx);
      sum = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
      for (; j < c; ++j) sum += expf(s[j] - mx);
    } else {
      sum = 0.f;
      for (int j = 0; j < c; ++j) sum += expf(s[j] - mx);
    }
    for (int j = 0; j < c; ++j) {
      const float p = expf(s[j] - mx) / sum;
      if (j == 0 || p > best) {
        best = p;
        arg = j;
      }
    }
  } else {
    best = s[0];
    for (int j = 1; j < c; ++j)
      if (s[j] > best) {
        best = s[j];
        arg = j;
      }
  }
  states[i] = best >= threshold ? arg : -1;
  if (top) top[i] = best;
}

hipError_t launch_scores_to_states(const float *logits, int n, int c, int softmax, float threshold, int *states, float *top,
                                   hipStream_t s) {
  if (!logits || !states || n <= 0 || c <= 0) return hipErrorInvalidValue;
  TSM_KLAUNCH(scores_to_states_kernel, dim3((n + 63) / 64), dim3(64), 0, s, logits, n, c, softmax, threshold, states, top);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// preprocess_image: the per-frame transform of the reference's IMAGE model (utils/inference_count.py:27-34: ToPILImage ->
// Resize(256) -> CenterCrop(224) -> ToTensor -> Normalize), i.e. Pillow's ImagingResample for 8-bit channels with the
// bilinear (triangle) filter: an antialiased horizontal pass rounded to uint8, then a vertical pass over those uint8 values,
// each u8 = clamp((2^21 + sum(pixel * k)) >> 22, 0, 255) with int32 weights the HOST computed in double (bounds + weights per
// output index of the crop window: transform.py::pil_resample_tables).  The kernel is integer arithmetic up to the final
// normalisation, which is what makes it Pillow's result to the bit.
// One workgroup per (frame, band of `band` output rows):
//   phase 1  the horizontally resampled uint8 rows the band's vertical support needs -> LDS (only the crop window's columns,
//            only their taps are read); a thread per (row, column), three channels each;
//   phase 2  the vertical pass from LDS, (u8 / 255 - mean) / std in fp32 (true divisions: the value is NumPy's to the bit),
//            packed as preprocess_kernel packs; a thread per output group.
// LDS rows are plain byte rows [rows][crop * 3, padded to 4 bytes]: in both phases the lanes of a wave walk consecutive columns
// of ONE row, i.e. consecutive bytes -- at most 192 contiguous bytes = 48 of the 64 banks per wave access, lanes that share a
// dword share its bank AND its address (a broadcast, not a conflict).  The rounding to uint8 between the passes is why a row
// costs one byte per channel here and why there are two real passes.
// A pass whose axis keeps its size is skipped (hk / vk == nullptr), as Pillow skips it: phase 1 then copies, phase 2 reads its
// own row.  TOTAL in the tables (device memory, no host check sees them): every bound is clamped into the frame / the rows in
// LDS before it is used, so for ANY table contents the kernel reads only inside `src` and its own LDS rows.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
__device__ __forceinline__ unsigned clip8(unsigned acc) {
  const int v = (int)acc >> 22;          // (arithmetic shift: Pillow's clip8 floors a negative sum, then clamps it to 0)
  return (unsigned)clampi(v, 0, 255);
}

__global__ void __launch_bounds__(256) preprocess_image_kernel(const ImagePreprocParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char img_rows[];
  const int nb = (p.crop + p.band - 1) / p.band;
  const int64_t f = blockIdx.x / nb;
  const int r0 = (int)(blockIdx.x - f * nb) * p.band;
  const int r1 = r0 + p.band < p.crop ? r0 + p.band : p.crop;
  // source rows [y0, y0 + nrows) under the band's vertical support
  int y0, nrows;
  if (p.vk) {
    y0 = clampi(p.vb[2 * r0], 0, p.h - 1);
    const int yend = clampi(p.vb[2 * (r1 - 1)] + p.vb[2 * (r1 - 1) + 1], y0 + 1, p.h);
    nrows = yend - y0 < p.rows_cap ? yend - y0 : p.rows_cap;
  } else {
    y0 = p.top + r0;
    nrows = r1 - r0;
  }
  const unsigned char *frame = p.src + f * (int64_t)p.h * p.w * 3;
  for (int i = threadIdx.x; i < nrows * p.crop; i += 256) {
    const int r = i / p.crop, cx = i - r * p.crop;
    const unsigned char *row = frame + (int64_t)(y0 + r) * p.w * 3;
    unsigned char *o = img_rows + r * p.stride + cx * 3;
    if (p.hk) {
      const int xmin = clampi(p.hb[2 * cx], 0, p.w - 1);
      const int room = p.w - xmin < p.ksx ? p.w - xmin : p.ksx;
      const int cnt = clampi(p.hb[2 * cx + 1], 0, room);
      const int *k = p.hk + (int64_t)cx * p.ksx;
      const unsigned char *q = row + xmin * 3;
      unsigned s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
      for (int t = 0; t < cnt; ++t) {
        const unsigned kv = (unsigned)k[t];
        s0 += q[3 * t] * kv;
        s1 += q[3 * t + 1] * kv;
        s2 += q[3 * t + 2] * kv;
      }
      o[0] = (unsigned char)clip8(s0);
      o[1] = (unsigned char)clip8(s1);
      o[2] = (unsigned char)clip8(s2);
    } else {
      const unsigned char *q = row + (p.left + cx) * 3;
      o[0] = q[0];
      o[1] = q[1];
      o[2] = q[2];
    }
  }
  __syncthreads();
  const int px = p.out_mode >= 2 ? 2 : 1;
  const int wg = (p.crop + px - 1) / px;
  for (int i = threadIdx.x; i < (r1 - r0) * wg; i += 256) {
    const int ry = i / wg, gx = i - ry * wg;
    const int cy = r0 + ry;
    int ymin = ry, cnt = 1;
    const int *k = nullptr;
    if (p.vk) {
      ymin = clampi(p.vb[2 * cy] - y0, 0, nrows - 1);
      const int room = nrows - ymin < p.ksy ? nrows - ymin : p.ksy;
      cnt = clampi(p.vb[2 * cy + 1], 0, room);
      k = p.vk + (int64_t)cy * p.ksy;
    }
    float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int x = gx * px + q;
      if (q >= px || x >= p.crop) continue;
      const unsigned char *col = img_rows + ymin * p.stride + x * 3;
      unsigned u[3];
      if (k) {
        unsigned s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
        for (int t = 0; t < cnt; ++t) {
          const unsigned kv = (unsigned)k[t];
          const unsigned char *e = col + t * p.stride;
          s0 += e[0] * kv;
          s1 += e[1] * kv;
          s2 += e[2] * kv;
        }
        u[0] = clip8(s0);
        u[1] = clip8(s1);
        u[2] = clip8(s2);
      } else {
        u[0] = col[0];
        u[1] = col[1];
        u[2] = col[2];
      }
#pragma unroll
      for (int c = 0; c < 3; ++c) v[4 * q + c] = ((float)u[c] / 255.0f - kMean[c]) / kStd[c];
    }
    const int64_t g = (f * p.crop + cy) * wg + gx;       // output group, as preprocess_rows numbers them
    store_pixel_group(p.dst, p.out_mode, p.crop, f, cy, gx, g, v);
  }
}

// LDS rows a band of `band` output rows can need: ymin(first) >= c0 - support - 0.5 and yend(last) <= c1 + support + 0.5 with
// c1 - c0 = (band - 1) * scale, so the span is at most (band - 1) * scale + 2 * support + 1 rows.
static int image_rows_cap(int band, int in, int out) {
  const double scale = (double)in / out, support = scale < 1.0 ? 1.0 : scale;
  return (int)((band - 1) * scale + 2.0 * support) + 2;
}

hipError_t launch_preprocess_image(ImagePreprocParams p, hipStream_t s) {
  if (!p.src || !p.dst || p.n <= 0 || p.nh <= 0 || p.nw <= 0 || !crop_window_ok(p) || p.out_mode < 0 || p.out_mode > 3)
    return hipErrorInvalidValue;
  // a pass without tables copies: legal only where that axis keeps its size (the crop window then lies inside the frame)
  if ((!p.hk && p.nw != p.w) || (!p.vk && p.nh != p.h) || (p.hk && (!p.hb || p.ksx <= 0)) || (p.vk && (!p.vb || p.ksy <= 0)))
    return hipErrorInvalidValue;
  p.stride = (p.crop * 3 + 3) & ~3;
  // the band height: 8 output rows unless the rows under their support do not fit 64 KB of LDS (a > 9x downscale at crop 224)
  for (p.band = 8;; p.band /= 2) {
    p.rows_cap = p.vk ? image_rows_cap(p.band, p.h, p.nh) : p.band;
    if ((int64_t)p.rows_cap * p.stride <= kImageMaxLds) break;
    if (p.band == 1) return hipErrorNotSupported;
  }
  const int64_t blocks = (int64_t)p.n * ((p.crop + p.band - 1) / p.band);
  if (blocks > 0x7fffffff) return hipErrorInvalidValue;
  TSM_KLAUNCH(preprocess_image_kernel, dim3((unsigned)blocks), dim3(256), (size_t)p.rows_cap * p.stride, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// preprocess_image_windows: preprocess_image over windows of DIFFERENT frame sizes (tsm_preprocess_windows with person_crop =
// TSM_WINDOWS_IMAGE), one launch from raw frames to the engine's packed input in batch order -- a step of ImageStreamBatcher.
// Window c's 8-dword descriptor {off_lo, off_hi, h, w, tab_lo, tab_hi, -, -} says where its n_segment contiguous frames and the
// coefficient block of its geometry (transform.image_tables' layout) start in the arena.  The host sees neither the table nor
// the sizes, so the launch has a FIXED dynamic LDS size (kImageMaxLds) and a grid-stride loop over the work items (window,
// frame, group of 8 output rows); per item the workgroup
//   * reads the descriptor and forms verdict and geometry (tsm_host::image_window_ok: int64, total in the eight words) BEFORE
//     any address exists; an invalid window reads nothing and its rows are the normalised zero frame;
//   * picks its own band -- 8, 4, 2 or 1 output rows, the largest whose rows under the vertical support fit the LDS -- and runs
//     preprocess_image_kernel's two passes per band: horizontal, rounded to uint8, into LDS byte rows (the same row layout, so
//     its bank behaviour), then vertical from LDS, (u8 / 255 - mean) / std, store_pixel_group.
// Integer arithmetic up to the final normalisation: a row does not depend on the band, the item or the grid, and equals
// preprocess_image_kernel's row for that frame bit for bit.  Src = Nv12: a source pixel is converted as it is read
// (Taps<Nv12>::pixel), which is tsm_preprocess_image on the converted frame.  TOTAL in the table contents as well: every bound
// is clamped -- in 64 bits where two table words meet -- into the frame / the rows in LDS before it is used.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int clampl(int64_t v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : (int)v); }

template <typename Src>
__global__ void __launch_bounds__(256) preprocess_image_windows_kernel(const WindowPreprocParams p) {
  extern __shared__ __attribute__((aligned(16))) unsigned char win_rows[];
  const int crop = p.crop, stride = tsm_host::image_row_stride(crop);
  const int nb8 = (crop + 7) / 8;
  const int px = p.out_mode >= 2 ? 2 : 1;
  const int wg = (crop + px - 1) / px;
  const int64_t total = (int64_t)p.n_windows * p.n_segment * nb8;
  for (int64_t item = blockIdx.x; item < total; item += gridDim.x) {
    const int64_t f = item / nb8;                       // output frame: (window, segment)
    const int g0 = (int)(item - f * nb8) * 8;
    const int g1 = g0 + 8 < crop ? g0 + 8 : crop;
    const int64_t c = f / p.n_segment;
    const int k = (int)(f - c * p.n_segment);
    typedef int desc_t __attribute__((ext_vector_type(4)));         // (16-byte aligned: the launcher checks the table's base)
    const desc_t *dp = reinterpret_cast<const desc_t *>(p.desc) + c * 2;
    const desc_t lo = dp[0], hi = dp[1];
    const int32_t d[tsm_host::kWindowDescWords] = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    tsm_host::ImageWindow win;
    if (!tsm_host::image_window_ok(d, p.n_segment, p.src_yuv == 1, p.arena_bytes, p.resize, crop, kImageMaxLds, &win)) {
      for (int i = threadIdx.x; i < (g1 - g0) * wg; i += 256) {
        const int ry = i / wg, gx = i - ry * wg;
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        zero_frame_pixel(v);
        if (px == 2 && gx * 2 + 1 < crop) zero_frame_pixel(v + 4);
        store_pixel_group(p.dst, p.out_mode, crop, f, g0 + ry, gx, (f * crop + g0 + ry) * wg + gx, v);
      }
      continue;
    }
    const int h = d[2], w = d[3];
    const Taps<Src> frame = Taps<Src>::of(static_cast<const char *>(p.arena) + win.off, k, h, w, p.nv12);
    const int *tab = reinterpret_cast<const int *>(static_cast<const char *>(p.arena) + win.tab);
    const int *hb = win.ksx ? tab : nullptr, *hk = tab + 2 * (int64_t)crop;
    const int *vb = win.ksy ? tab + win.hwords : nullptr, *vk = tab + win.hwords + 2 * (int64_t)crop;
    const int ksx = win.ksx, ksy = win.ksy;
    for (int r0 = g0; r0 < g1; r0 += win.band) {
      const int r1 = r0 + win.band < g1 ? r0 + win.band : g1;
      // source rows [y0, y0 + nrows) under the band's vertical support
      int y0, nrows;
      if (vb) {
        y0 = clampi(vb[2 * r0], 0, h - 1);
        const int yend = clampl((int64_t)vb[2 * (r1 - 1)] + vb[2 * (r1 - 1) + 1], y0 + 1, h);
        nrows = yend - y0 < win.rows_cap ? yend - y0 : win.rows_cap;
      } else {
        y0 = win.g.top + r0;
        nrows = r1 - r0;
      }
      for (int i = threadIdx.x; i < nrows * crop; i += 256) {
        const int r = i / crop, cx = i - r * crop;
        unsigned char *o = win_rows + r * stride + cx * 3;
        unsigned u[3];
        if (hb) {
          const int xmin = clampi(hb[2 * cx], 0, w - 1);
          const int room = w - xmin < ksx ? w - xmin : ksx;
          const int cnt = clampi(hb[2 * cx + 1], 0, room);
          const int *kx = hk + (int64_t)cx * ksx;
          unsigned s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
          for (int t = 0; t < cnt; ++t) {
            const unsigned kv = (unsigned)kx[t];
            frame.pixel(y0 + r, xmin + t, u);
            s0 += u[0] * kv;
            s1 += u[1] * kv;
            s2 += u[2] * kv;
          }
          u[0] = clip8(s0);
          u[1] = clip8(s1);
          u[2] = clip8(s2);
        } else {
          frame.pixel(y0 + r, win.g.left + cx, u);
        }
        o[0] = (unsigned char)u[0];
        o[1] = (unsigned char)u[1];
        o[2] = (unsigned char)u[2];
      }
      __syncthreads();
      for (int i = threadIdx.x; i < (r1 - r0) * wg; i += 256) {
        const int ry = i / wg, gx = i - ry * wg;
        const int cy = r0 + ry;
        int ymin = ry, cnt = 1;
        const int *ky = nullptr;
        if (vb) {
          ymin = clampl((int64_t)vb[2 * cy] - y0, 0, nrows - 1);
          const int room = nrows - ymin < ksy ? nrows - ymin : ksy;
          cnt = clampi(vb[2 * cy + 1], 0, room);
          ky = vk + (int64_t)cy * ksy;
        }
        float v[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int q = 0; q < 2; ++q) {
          const int x = gx * px + q;
          if (q >= px || x >= crop) continue;
          const unsigned char *col = win_rows + ymin * stride + x * 3;
          unsigned u[3];
          if (ky) {
            unsigned s0 = 1u << 21, s1 = 1u << 21, s2 = 1u << 21;
            for (int t = 0; t < cnt; ++t) {
              const unsigned kv = (unsigned)ky[t];
              const unsigned char *e = col + t * stride;
              s0 += e[0] * kv;
              s1 += e[1] * kv;
              s2 += e[2] * kv;
            }
            u[0] = clip8(s0);
            u[1] = clip8(s1);
            u[2] = clip8(s2);
          } else {
            u[0] = col[0];
            u[1] = col[1];
            u[2] = col[2];
          }
#pragma unroll
          for (int ch = 0; ch < 3; ++ch) v[4 * q + ch] = ((float)u[ch] / 255.0f - kMean[ch]) / kStd[ch];
        }
        store_pixel_group(p.dst, p.out_mode, crop, f, cy, gx, (f * crop + cy) * wg + gx, v);
      }
      __syncthreads();          // (the next band, or the next item, overwrites the rows this one still reads)
    }
  }
}

hipError_t launch_preprocess_image_windows(const WindowPreprocParams &p, hipStream_t s) {
  if (!p.arena || !p.dst || !p.desc || (reinterpret_cast<uintptr_t>(p.arena) & 15) != 0 || (reinterpret_cast<uintptr_t>(p.desc) & 15) != 0 ||
      p.arena_bytes <= 0 || p.n_windows <= 0 || p.n_segment <= 0 || p.resize <= 0 || p.crop <= 0 || p.out_mode < 0 || p.out_mode > 3 ||
      p.crop > p.resize)
    return hipErrorInvalidValue;
  if (p.src_yuv > 1 || (!p.src_yuv && !p.src_is_u8) || p.crop > tsm_host::kImageMaxCrop) return hipErrorNotSupported;
  const unsigned grid = grid_for((int64_t)p.n_windows * p.n_segment * ((p.crop + 7) / 8) * 256, 8192);
  if (p.src_yuv)
    TSM_KLAUNCH(preprocess_image_windows_kernel<Nv12>, dim3(grid), dim3(256), (size_t)kImageMaxLds, s, p);
  else
    TSM_KLAUNCH(preprocess_image_windows_kernel<unsigned char>, dim3(grid), dim3(256), (size_t)kImageMaxLds, s, p);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// frame_votes: the image model's vote (utils/inference_count.py:221-231): per frame the FIRST arg-max of its logits (as
// numpy.argmax breaks ties), pushed into a queue of 7; state = sum(queue) >= 4.  The sum is over CLASS IDS, exactly as the
// reference's sum(que) is -- for two classes "at least 4 of the last 7 frames are class 1", for more classes whatever that
// sum gives.  A video spans many batches: hist_in holds the arg-max of the n_hist (0..6) frames before this batch, oldest
// first, hist_out [6] receives the last min(6, n_hist + n) of (history ++ this batch), -1 behind them.  One thread per frame: it takes the arg-max
// of its own row and of the up to six rows before it again (num_class is tiny) instead of waiting for other threads, so the
// whole vote is one launch with no ordering between workgroups; the thread of the last frame writes hist_out.  hist_in and
// hist_out must not alias (threads of other workgroups still read the old history).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int first_argmax(const float *s, int c) {
  float best = s[0];
  int arg = 0;
  for (int j = 1; j < c; ++j)
    if (s[j] > best) {
      best = s[j];
      arg = j;
    }
  return arg;
}

__global__ void __launch_bounds__(64) frame_votes_kernel(const float *__restrict__ logits, int n, int c,
                                                         const int *__restrict__ hist_in, int n_hist, int *__restrict__ pred,
                                                         int *__restrict__ state, int *__restrict__ hist_out) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  int last[7];       // arg-max of sequence positions i - 6 .. i (position < 0: the history; before it: nothing, -1)
  int sum = 0;
#pragma unroll
  for (int d = 0; d < 7; ++d) {
    const int j = i - 6 + d;
    int a = -1;
    if (j >= 0)
      a = first_argmax(logits + (size_t)j * c, c);
    else if (n_hist + j >= 0)
      a = hist_in[n_hist + j];
    last[d] = a;
    sum += a < 0 ? 0 : a;
  }
  pred[i] = last[6];
  state[i] = sum >= 4 ? 1 : 0;
  if (i == n - 1 && hist_out) {
    const int m = n_hist + n < 6 ? n_hist + n : 6;
#pragma unroll
    for (int d = 1; d < 7; ++d)          // (static register index, run-time slot: position n - 7 + d is slot d - (7 - m))
      if (d >= 7 - m) hist_out[d - (7 - m)] = last[d];
    for (int e = m; e < 6; ++e) hist_out[e] = -1;     // the slots behind the count: defined, and no class id
  }
}

hipError_t launch_frame_votes(const float *logits, int n, int c, const int *hist_in, int n_hist, int *pred, int *state,
                              int *hist_out, hipStream_t s) {
  if (!logits || !pred || !state || n <= 0 || c <= 0 || n_hist < 0 || n_hist > 6 || (n_hist > 0 && !hist_in) ||
      (hist_out && hist_out == hist_in))
    return hipErrorInvalidValue;
  TSM_KLAUNCH(frame_votes_kernel, dim3((n + 63) / 64), dim3(64), 0, s, logits, n, c, hist_in, n_hist, pred, state, hist_out);
  return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// top1_tally: the comparison of scripts/eval_classification.py on the device -- per row the FIRST arg-max of its logits
// (frame_votes' tie rule), compared with the row's label, counted per class: total[label] += 1, correct[label] += (pred ==
// label).  The reference's loop (:42-46) compares a logits row with the label and never increments class_total; this is its
// intent.  The counters ACCUMULATE over the batches of a dataset: the caller zeroes them once and reads them once, so a
// batch leaves 4 bytes per sample (pred) and nothing else to fetch.
// ONE workgroup of 1024 threads: the rows go round the threads (n x c is tiny: a batch of clips), the launch's own counts
// are LDS atomics, then thread c adds class c's two sums to the global counters with an ordinary load, add and (vector) store.
// Launches on one stream are ordered and a launch has one workgroup, so no two threads ever touch one global counter: no
// global atomic is needed.  TOTAL in the labels (device memory): a label outside [0, c) indexes nothing and is counted nowhere.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kTallyMaxClass) top1_tally_kernel(const float *__restrict__ logits,
                                                                    const int *__restrict__ labels, int n, int c,
                                                                    int *__restrict__ pred, int *__restrict__ correct,
                                                                    int *__restrict__ total) {
  __shared__ int n_correct[kTallyMaxClass], n_total[kTallyMaxClass];
  const int t = threadIdx.x;
  n_correct[t] = 0;
  n_total[t] = 0;
  __syncthreads();
  for (int i = t; i < n; i += kTallyMaxClass) {
    const int a = first_argmax(logits + (size_t)i * c, c);
    if (pred) pred[i] = a;
    const int l = labels[i];
    if (l >= 0 && l < c) {
      atomicAdd(&n_total[l], 1);
      if (a == l) atomicAdd(&n_correct[l], 1);
    }
  }
  __syncthreads();
  if (t < c) {
    correct[t] += n_correct[t];
    total[t] += n_total[t];
  }
}

hipError_t launch_top1_tally(const float *logits, const int *labels, int n, int c, int *pred, int *correct, int *total,
                             hipStream_t s) {
  if (!logits || !labels || !correct || !total || n <= 0 || c <= 0) return hipErrorInvalidValue;
  if (c > kTallyMaxClass) return hipErrorNotSupported;
  TSM_KLAUNCH(top1_tally_kernel, dim3(1), dim3(kTallyMaxClass), 0, s, logits, labels, n, c, pred, correct, total);
  return hipGetLastError();
}


// ---- launch trace (tests): which kernels did this thread launch? ---------------------------------------------------
namespace {
struct LaunchTrace {
  bool on = false;
  std::string text;
};
thread_local LaunchTrace g_trace;
}  // namespace

void note_launch(const char *kernel, const char *where, int reverse, const char *mark) {
  if (!g_trace.on) return;
  // "(conv_igemm<BM, BN, ...>)" as the launch site spells it; inside a template the enclosing function's
  // "[BM = 64, BN = 64, ...]" (clang's __PRETTY_FUNCTION__) resolves the names
  std::string k(kernel);
  if (!k.empty() && k.front() == '(' && k.back() == ')') k = k.substr(1, k.size() - 2);
  const char *with = where ? strstr(where, " [") : nullptr;
  g_trace.text += k;
  if (with) g_trace.text += with;
  if (mark) g_trace.text += mark;
  if (reverse > 0) g_trace.text += " [reverse]";
  g_trace.text += '\n';
}
void trace_launches(bool on) {
  g_trace.on = on;
  if (on) g_trace.text.clear();
}
const char *launch_trace() { return g_trace.text.c_str(); }

hipError_t lds_opt_in(const void *kernel, size_t bytes) {
  return hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

const DeviceInfo &device_info() {
  static std::mutex mu;
  static std::map<int, DeviceInfo> seen;
  int dev = 0;
  (void)hipGetDevice(&dev);
  std::lock_guard<std::mutex> lock(mu);
  auto it = seen.find(dev);
  if (it != seen.end()) return it->second;
  DeviceInfo di;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) di.n_cu = prop.multiProcessorCount;
  for (hipError_t st : {opt_in_bf16_256(), opt_in_ws(), opt_in_bneck(), opt_in_conv31(), opt_in_front()})
    if (st != hipSuccess && di.status == hipSuccess) di.status = st;
  return seen.emplace(dev, di).first->second;
}

}  // namespace tsm
