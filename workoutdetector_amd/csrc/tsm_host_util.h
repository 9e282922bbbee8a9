// Pure-host pieces of the engine: BatchNorm folding / weight packing, the bf16 storage-format converters, the
// segment-length rule, a conv layer's packed geometry and the shapes of its launch's parameter block (conv_shape_params),
// tsm_conv_op's argument rules (conv_op_check), the frame transforms' window and crop arithmetic, the NV12 conversion, the
// ConvNeXt engine's sizes, K orders and weight packing (cnx_*) and the TSM_TUNE_CACHE line parser.  (The launch rules themselves: tsm_conv_rules.h.)  No HIP types, so this header also compiles with plain
// g++: tests/host_sanitize.cpp builds it with -fsanitize=address,undefined, fuzzes the parser and drives conv_op_check over
// its refusals, its accepted forms and the ends of int32 (CPU only; GPU ASAN is not available on this pool).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/tsm_hip.h"
#include "tsm_conv_rules.h"

namespace tsm_host {

constexpr float kBnEps = 1e-5f;
using tsm::kPrecF32;   // the precision enumeration: tsm::ConvPrec (tsm_conv_rules.h)
using tsm::kPrecBf16x3;
using tsm::kPrecBf16;

// Long-K fp32 layers accumulate K in segments of ~16 K-steps (512 channels-taps) so that they can also run
// split-K (one workgroup per tile and segment) with bit-identical results when the batch is too small to
// fill the chip with whole-K tiles.  The choice depends on the layer only, never on the batch size.
inline int segment_len(int kp, int prec) {
  if (prec != kPrecF32) return 0;
  const int nk = kp / 32;
  if (nk < 32) return 0;
  const int nseg = nk / 16;   // (segments of 8 K-steps were measured in round 2: no gain at batch 1-4)
  return (nk + nseg - 1) / nseg;
}

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// The tail split of a segmented 64x64 launch (ConvParams::ksplit = 2, tile code bit kCodeTailK).  The conv_igemm SEG kernel keeps
// `wg_per_cu` (five) workgroups per CU resident, so a launch of ntm x ntn tiles runs in rounds of wg_per_cu * n_cu; when the last
// round is less than ~85 % full its tiles -- rounded DOWN to whole rows of tiles, so that the tail is a contiguous range of output
// rows -- run as (tile, K segment) pieces.  Returns the first tail tile (a multiple of ntn, in (0, ntm * ntn)), or 0 when the
// launch should stay whole-K: no whole round, no remainder worth splitting, or the segment sums [n_seg][tail rows][cout] do not
// fit `scratch_elems` floats.
inline long tail_split_point(long m_rows, int cout, int n_seg, int n_cu, size_t scratch_elems, int wg_per_cu = 5) {
  if (m_rows <= 0 || cout <= 0 || cout % 64 != 0 || n_seg < 2 || n_cu <= 0) return 0;
  const long ntn = cout / 64, ntm = (m_rows + 63) / 64, tiles = ntm * ntn, slots = (long)wg_per_cu * n_cu;
  const long rounds = tiles / slots, rem = tiles - rounds * slots;
  if (rounds < 1 || rem == 0 || rem * 100 > slots * 85) return 0;
  const long from = rounds * slots / ntn * ntn;
  if (from <= 0 || from >= tiles) return 0;
  const size_t tail_rows = (size_t)(m_rows - (from / ntn) * 64);
  if ((size_t)n_seg * tail_rows * (size_t)cout > scratch_elems) return 0;
  return from;
}

inline uint16_t f2bf(float f) {  // round to nearest even, like v_cvt_pk_bf16_f32
  uint32_t u;
  std::memcpy(&u, &f, 4);
  if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
  u += 0x7fffu + ((u >> 16) & 1u);
  return (uint16_t)(u >> 16);
}
inline float bf2f(uint16_t h) {
  const uint32_t u = (uint32_t)h << 16;
  float f;
  std::memcpy(&f, &u, 4);
  return f;
}
// fp32 -> bf16, two elements per float slot (the vector shrinks to half its length).
inline void to_bf16(std::vector<float> *v) {
  std::vector<float> out((v->size() + 1) / 2, 0.f);
  uint16_t *o = reinterpret_cast<uint16_t *>(out.data());
  for (size_t i = 0; i < v->size(); ++i) o[i] = f2bf((*v)[i]);
  v->swap(out);
}
// In place: every group of 8 consecutive floats becomes [hi x8 | lo x8] bf16 (32 bytes, same size).
inline void to_split(std::vector<float> *v) {
  uint16_t g[16];
  for (size_t i = 0; i + 8 <= v->size(); i += 8) {
    for (int e = 0; e < 8; ++e) {
      const float x = (*v)[i + e];
      g[e] = f2bf(x);
      g[8 + e] = f2bf(x - bf2f(g[e]));
    }
    std::memcpy(v->data() + i, g, 32);
  }
}

// Stem weights for the bf16 formats, whose input is stored as pixel pairs (tsm_ops.hip, pack_input_kernel):
// K = (ky, pair j, pixel-in-pair q, c4) = 7 x 4 x 2 x 4 = 224, covering pixels 2ox-4 .. 2ox+3, i.e. kx = 2j + q - 1
// (kx = -1 and c = 3 carry zero weights).
inline void fold_and_pack_stem_pairs(const float *w, const float *gamma, const float *beta, const float *mean,
                              const float *var, int cout, int kp, std::vector<float> *wp, std::vector<float> *bias) {
  wp->assign((size_t)cout * kp, 0.f);
  bias->resize(cout);
  for (int o = 0; o < cout; ++o) {
    const float scale = gamma[o] / std::sqrt(var[o] + kBnEps);
    (*bias)[o] = beta[o] - mean[o] * scale;
    float *dst = wp->data() + (size_t)o * kp;
    for (int c = 0; c < 3; ++c)
      for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx) {
          const int j = (kx + 1) >> 1, q = (kx + 1) & 1;
          dst[((ky * 4 + j) * 2 + q) * 4 + c] = w[(((size_t)o * 3 + c) * 7 + ky) * 7 + kx] * scale;
        }
  }
}

// Fold BN into the conv and pack OIHW -> [Cout][Kp], K = (ky, kx, c) with c padded to cp.
inline void fold_and_pack(const float *w, const float *gamma, const float *beta, const float *mean,
                   const float *var, int cout, int cin, int k, int cp, int kp, std::vector<float> *wp,
                   std::vector<float> *bias) {
  wp->assign((size_t)cout * kp, 0.f);
  bias->resize(cout);
  for (int o = 0; o < cout; ++o) {
    const float scale = gamma[o] / std::sqrt(var[o] + kBnEps);
    (*bias)[o] = beta[o] - mean[o] * scale;
    float *dst = wp->data() + (size_t)o * kp;
    for (int c = 0; c < cin; ++c)
      for (int ky = 0; ky < k; ++ky)
        for (int kx = 0; kx < k; ++kx)
          dst[(ky * k + kx) * cp + c] = w[(((size_t)o * cin + c) * k + ky) * k + kx] * scale;
  }
}

// Bottleneck.conv3 + the downsample branch as ONE GEMM over K = [conv3's K | the downsample's K]: row o of the fused matrix is
// row o of each packed fp32 matrix (fold_and_pack) side by side, and the bias is the two folded biases summed in fp32.
inline void concat_k_pair(const std::vector<float> &w1, const std::vector<float> &b1, int kp1, const std::vector<float> &w2,
                          const std::vector<float> &b2, int kp2, int cout, std::vector<float> *wf, std::vector<float> *bf) {
  const int kpf = kp1 + kp2;
  wf->assign((size_t)cout * kpf, 0.f);
  bf->resize(cout);
  for (int o = 0; o < cout; ++o) {
    std::memcpy(&(*wf)[(size_t)o * kpf], &w1[(size_t)o * kp1], kp1 * sizeof(float));
    std::memcpy(&(*wf)[(size_t)o * kpf + kp1], &w2[(size_t)o * kp2], kp2 * sizeof(float));
    (*bf)[o] = b1[o] + b2[o];
  }
}

// A 1x1 conv WITH a bias [cout][cin] -> rows [row0, row0 + cout) of the packed matrix [rows][kp] and of the bias vector (both
// sized by the caller).  gamma == nullptr: no BatchNorm behind it -- the scale is exactly 1, weights and bias are copied
// bit for bit (the non-local block's theta / phi / g).  Otherwise BN(conv(x) + b) = conv(x) * s + (beta + (b - mean) * s) with
// s = gamma / sqrt(var + eps) (its W).
inline void fold_and_pack_bias(const float *w, const float *cbias, const float *gamma, const float *beta, const float *mean,
                               const float *var, int cout, int cin, int kp, int row0, std::vector<float> *wp,
                               std::vector<float> *bias) {
  for (int o = 0; o < cout; ++o) {
    float *dst = wp->data() + (size_t)(row0 + o) * kp;
    if (!gamma) {
      std::memcpy(dst, w + (size_t)o * cin, (size_t)cin * sizeof(float));
      (*bias)[row0 + o] = cbias[o];
      continue;
    }
    const float scale = gamma[o] / std::sqrt(var[o] + kBnEps);
    for (int c = 0; c < cin; ++c) dst[c] = w[(size_t)o * cin + c] * scale;
    (*bias)[row0 + o] = beta[o] + (cbias[o] - mean[o]) * scale;
  }
}

// ---- non-local blocks (TSM's make_non_local: NL3DWrapper around every other block of layer2 and layer3) ---------------------
// layer and block as in the state-dict key "layer<layer>.<block>": layer2.{0, 2} and layer3.{0, 2, 4} of a [3, 4, 6, 3] backbone.
inline bool nonlocal_wrapped(int layer, int block) { return (layer == 2 || layer == 3) && block % 2 == 0; }
// MaxPool3d((1, 2, 2)): floor mode, no padding -- a last odd row / column is dropped; 0 when nothing is left.
inline int pool2_size(int h) { return h > 0 ? h / 2 : 0; }
// Positions of one clip: queries T * h * w, keys T * (h / 2) * (w / 2); -1 when the product leaves int32 (the attention
// kernel's nq / nk are ints) or a size is not positive.
inline int64_t nonlocal_positions(int T, int h, int w) {
  if (T <= 0 || h <= 0 || w <= 0) return -1;
  const int64_t lim = (int64_t)1 << 31, th = (int64_t)T * h;   // (each factor < 2^31: no product here leaves int64)
  return th >= lim || th * w >= lim ? -1 : th * w;
}
inline int64_t nonlocal_keys(int T, int h, int w) { return nonlocal_positions(T, pool2_size(h), pool2_size(w)); }
// Tiles of `tile` rows that cover n rows (the attention kernel's query tiles per clip and key tiles per query tile).
inline int64_t tiles_over(int64_t n, int tile) { return n <= 0 || tile <= 0 ? 0 : (n + tile - 1) / tile; }

// ---- temporal pool (TSM's make_temporal_pool: TemporalPool around layer2) -----------------------------------------------------
// max_pool3d over time, kernel 3, stride 2, padding 1, per clip: T frames -> T / 2.  -1 for a T the engine does not pool
// (not positive, or odd: the original's n_segment_list = [T, T // 2, ...] and its view(-1, T // 2, ...) assume an even T).
inline int temporal_pool_segments(int T) { return T > 0 && T % 2 == 0 ? T / 2 : -1; }
// The source frames of output frame t_out of a T-frame clip: {2 t_out - 1, 2 t_out, 2 t_out + 1} cut to [0, T), inclusive ends;
// first > last when t_out is no output frame of such a clip.
struct PoolWindow {
  int first, last;
};
inline PoolWindow temporal_pool_window(int T, int t_out) {
  if (temporal_pool_segments(T) < 0 || t_out < 0 || t_out >= T / 2) return {0, -1};
  const int64_t lo = 2 * (int64_t)t_out - 1, hi = 2 * (int64_t)t_out + 1;
  return {(int)(lo < 0 ? 0 : lo), (int)(hi > T - 1 ? T - 1 : hi)};
}
// Why an engine of this precision, shift flag, segment count and non-local flag cannot pool; nullptr when it can.
inline const char *temporal_pool_refusal(int prec, int is_shift, int T, int non_local) {
  if (prec == kPrecBf16)
    return "the temporal pool runs in TSM_DTYPE_F32 and TSM_DTYPE_BF16X3 only (the bf16 cross-block and whole-block kernels tile over all T frames of a clip)";
  if (!is_shift) return "the temporal pool needs is_shift = 1 (make_temporal_pool is a branch of make_temporal_shift)";
  if (temporal_pool_segments(T) < 0) return "the temporal pool needs an even num_segments";
  if (non_local) return "the temporal pool and the non-local blocks exclude each other (the non-local wrapper assumes one segment count)";
  return nullptr;
}

// In the engine's storage format: fp32 as it is, split-bf16 in place, bf16 at half the length.
inline void to_storage(std::vector<float> *v, int prec) {
  if (prec == kPrecBf16x3) to_split(v);
  if (prec == kPrecBf16) to_bf16(v);
}

// ---- one conv layer: geometry and tsm_conv_op's rules, shared by the engine (build_topology) and the per-op conv ------------
inline int prec_of_dtype(int dtype) {   // tsm_dtype -> precision, -1 for anything else
  return dtype == TSM_DTYPE_F32 ? kPrecF32 : dtype == TSM_DTYPE_BF16X3 ? kPrecBf16x3 : dtype == TSM_DTYPE_BF16 ? kPrecBf16 : -1;
}
// Why tsm_create refuses a shift_div for an engine of this precision; nullptr when it takes it.  fold = channels / shift_div must be
// whole 16-byte groups of the narrowest shifted tensor (64 channels): 4 channels of fp32, 8 of the bf16 formats.  1 is taken:
// fold = channels, every channel reads frame t + 1 and the t - 1 group is empty (the reference's slicing).
inline const char *shift_div_refusal(int shift_div, int prec) {
  if (shift_div <= 0 || 64 % shift_div != 0 || (64 / shift_div) % 4 != 0)
    return "shift_div must be 1, 2, 4, 8 or 16 for TSM_DTYPE_F32 and 1, 2, 4 or 8 for the bf16 formats (fold = channels / shift_div in whole 4-channel groups)";
  if (prec != kPrecF32 && (64 / shift_div) % 8 != 0)
    return "the bf16 formats shift whole 8-channel groups (fold % 8 == 0): shift_div must be 1, 2, 4 or 8";
  return nullptr;
}
// Why an engine of this shift flag and shift_div cannot take this placement; nullptr when it can.  Block placement shifts the
// identity and the downsample operand, whose launches need both channel groups inside the tensor (conv_args_refused: 2 * fold
// <= channels): at shift_div 1 every forward would be refused, so the placement is refused up front.
inline const char *shift_place_refusal(int place, int is_shift, int shift_div) {
  if (place != 0 && place != 1) return "place must be 0 (blockres) or 1 (block)";
  if (place == 1 && is_shift && shift_div == 1)
    return "block placement needs shift_div >= 2: its shifted identity and downsample launches take 2 * fold <= channels (shift_div 1 runs in blockres placement only)";
  return nullptr;
}
inline int packed_layout_of(int prec) {   // the packed device-memory clip layout an engine of that precision consumes in place
  return prec == kPrecF32 ? TSM_LAYOUT_NTHWC4 : prec == kPrecBf16x3 ? TSM_LAYOUT_NTHWC8S : TSM_LAYOUT_NTHWC8B;
}

// Output size of a k x k conv with padding k / 2 (k odd; also the 3x3 max-pool) at `stride` > 0.  64-bit inside: total for h >= 1.
inline int conv_out_size(int h, int k, int stride) { return (int)(((int64_t)h + 2 * (k / 2) - k) / stride + 1); }

struct LayerGeom {
  int cp = 0;    // channel count the kernel sees (stem: 3 -> 4)
  int kp = 0;    // padded K
  int kseg = 0;  // K-steps per accumulation segment (fp32 layers with long K, ConvParams::kseg_len); 0 = unsegmented
  bool stem_pairs = false;   // K in fold_and_pack_stem_pairs' order
};
// The packed geometry of a k x k conv over cin channels (k * k * cin + 63 fits an int).  K = (ky, kx, c) rounded up to the
// K-step of the format, 32 (bf16: 64); the 7x7 stem sees 4 channels, and in the bf16 formats, whose stride-2 stem reads
// pixel pairs, K = 7 rows x 4 pairs x 8.  Output channels and, beyond the stem's layout, the stride change nothing.
inline LayerGeom layer_geometry(int cin, int k, int stride, int prec) {
  LayerGeom g;
  g.stem_pairs = k == 7 && stride == 2 && prec != kPrecF32;
  g.cp = k == 7 ? 4 : cin;
  g.kp = round_up(g.stem_pairs ? 7 * 4 * 8 : k * k * g.cp, prec == kPrecBf16 ? 64 : 32);
  g.kseg = segment_len(g.kp, prec);
  return g;
}

inline int ilog2(int v) {
  int l = 0;
  while ((1 << l) < v) ++l;
  return l;
}

// The shapes of a conv launch's parameter block from its layer's packed geometry, on n frames of hi x wi pixels (the pointers,
// which the engine's make_params and set_second_source add, stay NULL).  `residual`: the launch adds one.
inline tsm::ConvParams conv_shape_params(const LayerGeom &g, int k, int stride, int cout, int n, int hi, int wi, bool relu, int T,
                                         int shift_div, int prec, bool residual) {
  tsm::ConvParams p{};
  p.prec = prec;
  p.N = n; p.Hi = hi; p.Wi = wi; p.C = g.cp; p.logC4 = ilog2(g.cp / 4);
  p.pad = k / 2; p.stride = stride;
  p.Ho = conv_out_size(hi, k, stride);
  p.Wo = conv_out_size(wi, k, stride);
  p.Cout = cout; p.Kp = g.kp; p.M = n * p.Ho * p.Wo; p.relu = relu ? 1 : 0;
  p.T = T; p.fold = T > 0 ? g.cp / shift_div : 0;
  p.kseg_len = residual ? 0 : g.kseg;   // (no layer with a residual has a long K; the per-op entry point refuses the pair)
  return p;
}
// A second source behind p's own K: one GEMM over K = [p's K | kp2], segmented by the whole K.  [N, hi2, wi2, c2], read at stride2.
inline void second_source_shape(tsm::ConvParams *p, int kp2, int c2, int hi2, int wi2, int stride2) {
  p->K1 = p->Kp;
  p->Kp += kp2;
  p->kseg_len = segment_len(p->Kp, p->prec);
  p->C2 = c2; p->Hi2 = hi2; p->Wi2 = wi2; p->stride2 = stride2;
}

// conv_op_check's verdict on a tsm_conv_args: TSM_OK and what tsm_conv_op derives from the arguments, or the refusal.
struct ConvOpPlan {
  int status = TSM_OK;         // the refusal's tsm_status
  const char *message = "";    // and its text
  int prec = 0;
  bool stem = false, dual = false;
  int T = 0, fold = 0;         // segments of the shift (0: none) and the channels it moves each way
  int ho = 0, wo = 0;
  LayerGeom geo;               // the main conv's cp, kp
  int kp2 = 0;                 // the second source's padded K (0: none)
  int kseg = 0;                // a single source's K-steps per segment where the code asks for it (kCodeOpSegmented); else 0
  // element counts, each below 2^31: output rows, the staged input (stem: 8 per pixel), the output, the second source, [cout][kp + kp2]
  int64_t rows = 0, x_elems = 0, y_elems = 0, x2_elems = 0, w_elems = 0;
};

// tsm_conv_args.code only (TSM_CONV_CODE_SEGMENTED): a single fp32 source accumulates K in layer_geometry's segments, as the
// engine's add_conv(..., segmented = true) layers do.  Outside kCodeValid (below): tsm_conv_op takes it off before the code
// is checked, and no engine code, tsm_conv_tiles report or TSM_TUNE_CACHE line ever carries it.
constexpr int kCodeOpSegmented = 0x4000;

constexpr int64_t kInt31 = (int64_t)1 << 31;
// x * y of two counts in [0, 2^31], saturating at 2^31.
inline int64_t mul_sat31(int64_t x, int64_t y) { return x >= kInt31 || y >= kInt31 || x * y >= kInt31 ? kInt31 : x * y; }

// Every rule of tsm_conv_op, before its first HIP call: total for ANY argument values (pointers are compared with NULL, never
// read).  Sizes that the kernels' and the staging's 32-bit arithmetic cannot hold are TSM_ERR_CAPACITY, as in tsm_create.
inline ConvOpPlan conv_op_check(const tsm_conv_args *a) {
  ConvOpPlan p;
  auto refuse = [&p](int status, const char *message) { p.status = status; p.message = message; return p; };
  if (!a || a->struct_size != (int32_t)sizeof(tsm_conv_args)) return refuse(TSM_ERR_INVALID_ARG, "tsm_conv_args.struct_size must be sizeof(tsm_conv_args)");
  p.prec = prec_of_dtype(a->dtype);
  if (p.prec < 0) return refuse(TSM_ERR_UNSUPPORTED, "bad dtype");
  const bool x3 = p.prec != kPrecF32, bf16 = p.prec == kPrecBf16;   // x3: any non-fp32 storage format
  const int n = a->n, hi = a->hi, wi = a->wi, cin = a->cin, cout = a->cout, k = a->k, stride = a->stride, cin2 = a->cin2;
  const int fold_div = a->fold_div > 0 ? a->fold_div : 1;
  const bool residual = a->residual != nullptr;
  p.T = a->shift_segments > 0 ? a->shift_segments : 0;
  p.dual = a->x2 != nullptr;
  if (!a->x || !a->w || !a->gamma || !a->beta || !a->mean || !a->var || !a->y) return refuse(TSM_ERR_INVALID_ARG, "NULL pointer");
  if (n <= 0 || hi <= 0 || wi <= 0) return refuse(TSM_ERR_INVALID_ARG, "n, hi and wi must be positive");
  if (k != 1 && k != 3 && k != 7) return refuse(TSM_ERR_UNSUPPORTED, "k must be 1, 3 or 7");
  if (stride != 1 && stride != 2) return refuse(TSM_ERR_UNSUPPORTED, "stride must be 1 or 2");
  p.stem = k == 7;
  if (p.stem ? (cin != 3) : (cin < 32 || (cin & (cin - 1)) != 0)) return refuse(TSM_ERR_UNSUPPORTED, "cin must be 3 (k=7) or a power of two >= 32");
  if (bf16 && !p.stem && cin % 64 != 0) return refuse(TSM_ERR_UNSUPPORTED, "TSM_DTYPE_BF16 needs cin % 64 == 0");
  if (cout <= 0 || cout % 64 != 0) return refuse(TSM_ERR_UNSUPPORTED, "cout must be a multiple of 64");
  if (p.stem && (residual || p.dual || p.T > 0)) return refuse(TSM_ERR_INVALID_ARG, "the 7x7 stem has no residual, second source or shift");
  // What the shift moves: the input (0), or the identity (1: block placement) -- the residual, the second source, or for a
  // 1x1 at stride 2 (a BasicBlock's downsample) the input, which is that block's identity.
  if (a->shift_target != 0 && a->shift_target != 1) return refuse(TSM_ERR_INVALID_ARG, "shift_target must be 0 or 1");
  const bool strided_1x1 = k == 1 && stride != 1;
  if (a->shift_target == 1 && !residual && !p.dual && !strided_1x1)
    return refuse(TSM_ERR_INVALID_ARG, "shift_target 1 needs a residual, a second source or a 1x1 at stride 2");
  if (p.T > 0 && a->shift_target == 0) {
    if (residual) return refuse(TSM_ERR_INVALID_ARG, "a shifted input with a residual: no such launch (shift_target 1 shifts the residual)");
    if (p.dual) return refuse(TSM_ERR_INVALID_ARG, "a shifted first source with a second source: no such launch");
    if (strided_1x1) return refuse(TSM_ERR_INVALID_ARG, "a shifted 1x1 at stride 2 is the identity's (shift_target 1)");
  }
  p.ho = conv_out_size(hi, k, stride);
  p.wo = conv_out_size(wi, k, stride);
  if (p.dual) {
    if (k != 1) return refuse(TSM_ERR_UNSUPPORTED, "a second source needs a 1x1 main conv");
    if (residual) return refuse(TSM_ERR_INVALID_ARG, "a second source with a residual: no such launch");
    if (!a->w2 || !a->gamma2 || !a->beta2 || !a->mean2 || !a->var2) return refuse(TSM_ERR_INVALID_ARG, "NULL pointer (second source)");
    if (cin2 < 32 || (cin2 & (cin2 - 1)) != 0 || (bf16 && cin2 % 64 != 0))
      return refuse(TSM_ERR_UNSUPPORTED, "cin2 must be a power of two >= 32 (TSM_DTYPE_BF16: >= 64)");
    if (a->stride2 != 1 && a->stride2 != 2) return refuse(TSM_ERR_UNSUPPORTED, "stride2 must be 1 or 2");
    if (a->hi2 <= 0 || a->wi2 <= 0 || conv_out_size(a->hi2, 1, a->stride2) != p.ho || conv_out_size(a->wi2, 1, a->stride2) != p.wo)
      return refuse(TSM_ERR_INVALID_ARG, "the second source's output size must equal the main conv's");
  }
  if (p.T > 0) {
    const int shifted_c = a->shift_target == 0 ? cin : residual ? cout : p.dual ? cin2 : cin;
    p.fold = shifted_c / fold_div;
    if (n % p.T != 0) return refuse(TSM_ERR_INVALID_ARG, "n must be a whole number of T-frame clips");
    if (p.fold % (x3 ? 8 : 4) != 0)
      return refuse(TSM_ERR_UNSUPPORTED, x3 ? "the bf16 formats shift whole 8-channel groups: fold % 8 == 0" : "fp32 shifts whole 4-channel groups: fold % 4 == 0");
    if (2 * (int64_t)p.fold > shifted_c) return refuse(TSM_ERR_INVALID_ARG, "2 * fold exceeds the shifted tensor's channels");
  }
  if (p.stem && x3 && stride != 2) return refuse(TSM_ERR_UNSUPPORTED, "the bf16 formats implement the 7x7 stem for stride 2 only");
  if ((int64_t)k * k * cin + 63 + (p.dual ? (int64_t)cin2 + 63 : 0) > INT32_MAX)
    return refuse(TSM_ERR_CAPACITY, "the padded K (k * k * cin, plus cin2) must fit a 32-bit int");
  p.geo = layer_geometry(cin, k, stride, p.prec);
  p.kp2 = p.dual ? layer_geometry(cin2, 1, a->stride2, p.prec).kp : 0;
  if (a->code > 0 && (a->code & kCodeOpSegmented)) {   // the engine's segmented single-source form, where a kernel for it exists
    if (p.prec != kPrecF32) return refuse(TSM_ERR_INVALID_ARG, "a segmented conv is fp32 only");
    if (p.stem) return refuse(TSM_ERR_INVALID_ARG, "the 7x7 stem has no segmented form");
    if (residual) return refuse(TSM_ERR_INVALID_ARG, "a conv with a residual has no segmented form");
    if (p.dual) return refuse(TSM_ERR_INVALID_ARG, "a second source is segmented by its whole K already: the segmented bit is a single source's");
    if (k == 3 && p.T > 0) return refuse(TSM_ERR_INVALID_ARG, "a shifted 3x3 has no segmented form");
    if (p.geo.kseg == 0) return refuse(TSM_ERR_INVALID_ARG, "a segmented conv needs at least 32 K-steps (k * k * cin >= 1024)");
    p.kseg = p.geo.kseg;
  }
  p.rows = mul_sat31(mul_sat31(n, p.ho), p.wo);
  if (p.rows >= kInt31) return refuse(TSM_ERR_CAPACITY, "n * ho * wo (output rows) must stay below 2^31");
  p.x_elems = mul_sat31(mul_sat31(mul_sat31(n, hi), wi), p.stem ? 8 : cin);
  p.y_elems = mul_sat31(p.rows, cout);
  p.x2_elems = p.dual ? mul_sat31(mul_sat31(mul_sat31(n, a->hi2), a->wi2), cin2) : 0;
  p.w_elems = mul_sat31(cout, p.geo.kp + p.kp2);
  if (p.x_elems >= kInt31 || p.y_elems >= kInt31 || p.x2_elems >= kInt31 || p.w_elems >= kInt31)
    return refuse(TSM_ERR_CAPACITY, "the input, the output, the second source and the packed weights must each stay below 2^31 elements");
  return p;
}

// ---- hostile memory (tsm_conv_op's staging buffers; the engine under TSM_POISON=1) -----------------------------------------
// A guarded device buffer is [band | payload | slack + band]: the bands hold kPoisonWord (as fp32 a quiet NaN with a payload
// arithmetic never produces, as two bf16 two quiet NaNs, as an int32 no class id) and must still hold it after the launches --
// a stray store lands in owned memory and is reported, a stray read returns poison instead of a plausible leftover.  Band = one
// frame of the buffer (the reach of a wrong temporal-shift or halo index) rounded up to 512 bytes, at least 4 KiB; the payload
// keeps the 512-byte alignment of the allocation.
constexpr uint32_t kPoisonWord = 0x7FC07FC0u;
constexpr size_t kGuardAlign = 512, kGuardMinBand = 4096;

inline size_t guard_band_bytes(size_t frame_bytes) {
  const size_t r = (frame_bytes + kGuardAlign - 1) / kGuardAlign * kGuardAlign;
  return r < kGuardMinBand ? kGuardMinBand : r;
}

struct GuardLayout {
  size_t lead = 0;     // bytes of the band before the payload (= the payload's offset in the allocation)
  size_t payload = 0;  // bytes of the payload (a multiple of 4)
  size_t tail = 0;     // bytes behind the payload: the slack up to 512 bytes + the band after
  size_t total() const { return lead + payload + tail; }
};

inline GuardLayout guard_layout(size_t payload_bytes, size_t frame_bytes) {
  GuardLayout g;
  g.payload = (payload_bytes + 3) / 4 * 4;
  g.lead = guard_band_bytes(frame_bytes);
  g.tail = (g.payload + kGuardAlign - 1) / kGuardAlign * kGuardAlign - g.payload + g.lead;
  return g;
}

// Index of the first word of a band that no longer holds `fill`, or -1.
inline long guard_first_bad(const uint32_t *words, size_t n, uint32_t fill = kPoisonWord) {
  for (size_t i = 0; i < n; ++i)
    if (words[i] != fill) return (long)i;
  return -1;
}

// The message for word `idx` of the band before (`after` = false) or after the payload: the buffer, the side and the offset in
// elements of `elem_bytes` relative to the payload's first element (negative before it, >= its element count after it).
inline std::string guard_message(const std::string &name, const GuardLayout &g, bool after, size_t idx, size_t elem_bytes, uint32_t got) {
  const long long rel = after ? (long long)(g.payload + 4 * idx) : (long long)(4 * idx) - (long long)g.lead;   // bytes from the payload's start
  const long long eb = elem_bytes ? (long long)elem_bytes : 4;
  const long long elem = rel >= 0 ? rel / eb : -((-rel + eb - 1) / eb);
  char hex[16];
  std::snprintf(hex, sizeof hex, "0x%08x", got);
  return name + ": stray store into the band " + (after ? "after" : "before") + " the buffer, element offset " + std::to_string(elem) +
         (after ? " (" + std::to_string(rel - (long long)g.payload) + " bytes past its end)" : " (" + std::to_string(-rel) + " bytes before its start)") +
         ", the word there is " + hex;
}

// ---- frame transforms (tsm_preprocess*, tsm_gather_clips): the pure-integer parts of their argument checks -----------------
// torchvision's Resize(int) + CenterCrop(crop) of an h x w frame: the short side -> resize, the long side ->
// int(resize * long / short); the crop window starts at int(round((dim - crop) / 2)) with Python's round-half-to-even.
// False when the crop is larger than the resized frame.  h, w, resize, crop > 0.
struct CropGeometry {
  int nh, nw, top, left;
};
inline bool center_crop_geometry(int h, int w, int resize, int crop, CropGeometry *g) {
  if (h <= w) { g->nh = resize; g->nw = (int)((double)resize * w / h); }
  else { g->nh = (int)((double)resize * h / w); g->nw = resize; }
  if (crop > g->nh || crop > g->nw) return false;
  g->top = (int)std::nearbyint((g->nh - crop) / 2.0);
  g->left = (int)std::nearbyint((g->nw - crop) / 2.0);
  return true;
}

// ---- tsm_preprocess_windows: the per-window arithmetic its kernel runs, as pure-integer functions that compile for the host
// too, so that the kernel's bounds logic is tested on a CPU (tests/windows_host.cpp, under ASAN + UBSAN) before it runs on a GPU.
// center_crop_geometry in integers: the long side is resize * long / short in int64 (the double quotient above truncates to
// the same integer: a non-integral quotient lies at least 1 / 65535 from one, far outside a double's rounding of a product
// below 2^47), the crop starts at round-half-to-even of (dim - crop) / 2.  Equal to center_crop_geometry for h, w in
// 1 .. 65535.  False when the crop is larger than the resized frame or the long side does not fit an int32.
TSM_HOST_DEVICE inline bool center_crop_geometry_int(int h, int w, int resize, int crop, CropGeometry *g) {
  const int64_t lng = h <= w ? ((int64_t)resize * w) / h : ((int64_t)resize * h) / w;
  if (lng > INT32_MAX) return false;
  g->nh = h <= w ? resize : (int)lng;
  g->nw = h <= w ? (int)lng : resize;
  if (crop > g->nh || crop > g->nw) return false;
  const int dh = g->nh - crop, dw = g->nw - crop;       // a half rounds to the even neighbour: up only from an odd floor
  g->top = (dh >> 1) + (dh & (dh >> 1) & 1);
  g->left = (dw >> 1) + (dw & (dw >> 1) & 1);
  return true;
}

// One window of a tsm_preprocess_windows launch as its descriptor words say it: n_segment contiguous frames [h, w, 3] of
// elem_bytes (1 or 4) per channel, the first at byte `off` of an arena of arena_bytes (> 0); n_segment, resize, crop > 0.
// d = {off_lo, off_hi, h, w, top, left, bh, bw}.  True -- for ANY eight int32 words, and no intermediate leaves int64 -- only
// if off >= 0, off % 16 == 0, 1 <= h, w <= 65535 and off + n_segment * h * w * 3 * elem_bytes <= arena_bytes; with `center`
// the centre crop must also fit the resized frame, and *g is its geometry.  *off is set whenever the result is true.
constexpr int kWindowDescWords = 8, kWindowMaxSide = 65535;
TSM_HOST_DEVICE inline bool window_descriptor_ok(const int32_t d[kWindowDescWords], int n_segment, int elem_bytes, int64_t arena_bytes,
                                                 bool center, int resize, int crop, int64_t *off, CropGeometry *g) {
  const int64_t o = (int64_t)(((uint64_t)(uint32_t)d[1] << 32) | (uint32_t)d[0]);
  const int h = d[2], w = d[3];
  if (o < 0 || (o & 15) != 0 || h < 1 || h > kWindowMaxSide || w < 1 || w > kWindowMaxSide || o > arena_bytes) return false;
  const int64_t frame_bytes = (int64_t)h * w * 3 * elem_bytes;       // < 2^36
  int64_t bytes;
  if (__builtin_mul_overflow((int64_t)n_segment, frame_bytes, &bytes) || bytes > arena_bytes - o) return false;
  if (center && !center_crop_geometry_int(h, w, resize, crop, g)) return false;
  *off = o;
  return true;
}

// ---- NV12 frames (TSM_PIXEL_NV12_*): the integer arithmetic the frame-transform kernels run, as functions that compile for
// the host too (tests/nv12_host.cpp, under ASAN + UBSAN).  One frame is h * w luma bytes, then h / 2 rows of w bytes of
// interleaved (U, V) pairs, dense; h and w are even.  A 2x2 block of luma pixels shares one pair (nearest-neighbour chroma).
//   C = Y - y_off, D = U - 128, E = V - 128
//   R = clamp((cy C + crv E + 8192) >> 14),  G = clamp((cy C + cgu D + cgv E + 8192) >> 14),  B = clamp((cy C + cbu D + 8192) >> 14)
// in int32 (the largest magnitude is below 2^24), the coefficients round(x * 2^14) of the BT.601 / BT.709 matrices.
struct Nv12Coef {
  int32_t y_off, cy, crv, cgu, cgv, cbu;
};
constexpr int kNv12CoefWords = 6;   // a launch's parameter block carries the row as six plain words, in the struct's order
TSM_HOST_DEVICE inline Nv12Coef nv12_coef_of(const int32_t k[kNv12CoefWords]) { return {k[0], k[1], k[2], k[3], k[4], k[5]}; }
TSM_HOST_DEVICE inline bool pixel_is_nv12(int pixel) { return pixel >= TSM_PIXEL_NV12_BT601 && pixel <= TSM_PIXEL_NV12_BT709_FULL; }
// The coefficient row of an NV12 pixel code; false (and *k untouched) for any other code.
TSM_HOST_DEVICE inline bool nv12_coefficients(int pixel, Nv12Coef *k) {
  switch (pixel) {
    case TSM_PIXEL_NV12_BT601: *k = {16, 19077, 26149, -6419, -13320, 33050}; return true;
    case TSM_PIXEL_NV12_BT709: *k = {16, 19077, 29372, -3494, -8731, 34610}; return true;
    case TSM_PIXEL_NV12_BT601_FULL: *k = {0, 16384, 22970, -5638, -11700, 29032}; return true;
    case TSM_PIXEL_NV12_BT709_FULL: *k = {0, 16384, 25802, -3069, -7670, 30402}; return true;
    default: return false;
  }
}
// ---- The other YUV frame formats (TSM_PIXEL_I420_* .. TSM_PIXEL_UYVY_*): pixel code 32 + 4 f + c, f the layout below, c the
// coefficient row in the order of the NV12 codes.  All dense; the conversion is nv12_pixel_rgb on 8-bit samples.
//   I420  h * w Y bytes, then h/2 * w/2 U bytes, then h/2 * w/2 V bytes; a 2x2 block shares one U and one V byte.
//   YV12  I420 with the V plane before the U plane.
//   P010  NV12's arrangement in 16-bit little-endian samples, the 10 significant bits on top; a sample enters the formula as
//         its HIGH byte (word >> 8), the low byte is ignored: a P010 frame is the NV12 frame made of its high bytes.
//   YUYV  h rows of w/2 groups of the bytes (Y0, U, Y1, V): the two pixels of a group share U and V; rows share nothing.
//   UYVY  the same with the bytes (U, Y0, V, Y1).
// w is even everywhere, h too in the three 4:2:0 layouts.  P010, YUYV and UYVY frames are read in aligned 4-byte groups: the
// base is 4-byte aligned (every frame size of theirs is a multiple of 4).
enum YuvLayout { kYuvI420 = 0, kYuvYv12 = 1, kYuvP010 = 2, kYuvYuyv = 3, kYuvUyvy = 4, kYuvLayouts = 5 };
// The layout of a pixel code, -1 for every code outside TSM_PIXEL_I420_BT601 .. TSM_PIXEL_UYVY_BT709_FULL (NV12's included).
TSM_HOST_DEVICE inline int yuv_layout_of(int pixel) {
  return pixel >= TSM_PIXEL_I420_BT601 && pixel <= TSM_PIXEL_UYVY_BT709_FULL ? (pixel - TSM_PIXEL_I420_BT601) >> 2 : -1;
}
// The coefficient row of such a code (that of the NV12 code with the same c); false (and *k untouched) for any other code.
TSM_HOST_DEVICE inline bool yuv_coefficients(int pixel, Nv12Coef *k) {
  return yuv_layout_of(pixel) >= 0 && nv12_coefficients(TSM_PIXEL_NV12_BT601 + ((pixel - TSM_PIXEL_I420_BT601) & 3), k);
}
TSM_HOST_DEVICE inline bool yuv_is_420(int layout) { return layout <= kYuvP010; }
TSM_HOST_DEVICE inline bool yuv_sides_ok(int layout, int h, int w) {
  return h >= 1 && w >= 2 && (w & 1) == 0 && (!yuv_is_420(layout) || (h & 1) == 0);
}
// Bytes of one frame (sides as yuv_sides_ok has them, at most 65535: below 2^34) and the alignment its base needs.
TSM_HOST_DEVICE inline int64_t yuv_frame_bytes(int layout, int h, int w) {
  const int64_t hw = (int64_t)h * w;
  return layout == kYuvP010 ? hw * 3 : yuv_is_420(layout) ? hw / 2 * 3 : hw * 2;
}
TSM_HOST_DEVICE inline int yuv_alignment(int layout) { return layout >= kYuvP010 ? 4 : 1; }

// Bytes of one h x w frame of a pixel code (h, w in 1 .. 65535: below 2^36); -1 for an unknown code, or a YUV code with a
// side of the wrong parity.
TSM_HOST_DEVICE inline int64_t frame_bytes_of(int pixel, int h, int w) {
  if (h < 1 || w < 1) return -1;
  const int64_t hw = (int64_t)h * w;
  if (pixel == TSM_PIXEL_U8) return hw * 3;
  if (pixel == TSM_PIXEL_F32) return hw * 12;
  if (pixel_is_nv12(pixel)) return ((h | w) & 1) ? -1 : hw / 2 * 3;
  const int layout = yuv_layout_of(pixel);
  if (layout >= 0) return yuv_sides_ok(layout, h, w) ? yuv_frame_bytes(layout, h, w) : -1;
  return -1;
}
TSM_HOST_DEVICE inline int nv12_clamp255(int v) { return v < 0 ? 0 : v > 255 ? 255 : v; }
// One pixel: bytes (Y, U, V) -> rgb[3] in 0 .. 255.
TSM_HOST_DEVICE inline void nv12_pixel_rgb(const Nv12Coef &k, int Y, int U, int V, int rgb[3]) {
  const int c = k.cy * (Y - k.y_off) + 8192, d = U - 128, e = V - 128;
  rgb[0] = nv12_clamp255((c + k.crv * e) >> 14);
  rgb[1] = nv12_clamp255((c + k.cgu * d + k.cgv * e) >> 14);
  rgb[2] = nv12_clamp255((c + k.cbu * d) >> 14);
}
// Byte offsets in an h x w frame of luma pixel (y, x) and of the U byte of its chroma pair (V follows; the offset is even).
TSM_HOST_DEVICE inline int64_t nv12_luma_offset(int w, int64_t y, int64_t x) { return y * w + x; }
TSM_HOST_DEVICE inline int64_t nv12_chroma_offset(int h, int w, int64_t y, int64_t x) {
  return (int64_t)h * w + (y >> 1) * w + ((x >> 1) << 1);
}
// window_descriptor_ok for a window of NV12 frames: n_segment contiguous frames of 3 h w / 2 bytes, h and w even.
TSM_HOST_DEVICE inline bool nv12_window_descriptor_ok(const int32_t d[kWindowDescWords], int n_segment, int64_t arena_bytes, bool center,
                                                      int resize, int crop, int64_t *off, CropGeometry *g) {
  const int64_t o = (int64_t)(((uint64_t)(uint32_t)d[1] << 32) | (uint32_t)d[0]);
  const int h = d[2], w = d[3];
  if (o < 0 || (o & 15) != 0 || h < 2 || h > kWindowMaxSide || w < 2 || w > kWindowMaxSide || ((h | w) & 1) != 0 || o > arena_bytes)
    return false;
  const int64_t frame_bytes = (int64_t)h * w / 2 * 3;       // < 2^33
  int64_t bytes;
  if (__builtin_mul_overflow((int64_t)n_segment, frame_bytes, &bytes) || bytes > arena_bytes - o) return false;
  if (center && !center_crop_geometry_int(h, w, resize, crop, g)) return false;
  *off = o;
  return true;
}

// Byte offsets in an h x w frame of a YuvLayout of the 8-bit samples pixel (y, x) converts from: its Y, U and V (P010: the
// high bytes).  yuv_group_offset: the aligned 4 bytes that hold both chroma samples of the pixel -- and, in the packed
// layouts, both luma samples of its pair -- which the kernels load once (P010, YUYV, UYVY; the planar layouts have none).
TSM_HOST_DEVICE inline int64_t yuv_group_offset(int layout, int h, int w, int64_t y, int64_t x) {
  return layout == kYuvP010 ? (int64_t)h * w * 2 + (y >> 1) * w * 2 + ((x >> 1) << 2) : y * w * 2 + ((x >> 1) << 2);
}
TSM_HOST_DEVICE inline int64_t yuv_y_offset(int layout, int h, int w, int64_t y, int64_t x) {
  switch (layout) {
    case kYuvP010: return (y * w + x) * 2 + 1;
    case kYuvYuyv: return yuv_group_offset(layout, h, w, y, x) + ((x & 1) << 1);
    case kYuvUyvy: return yuv_group_offset(layout, h, w, y, x) + ((x & 1) << 1) + 1;
    default: return y * w + x;
  }
}
TSM_HOST_DEVICE inline int64_t yuv_u_offset(int layout, int h, int w, int64_t y, int64_t x) {
  const int64_t plane = (int64_t)(h >> 1) * (w >> 1);
  switch (layout) {
    case kYuvI420: return (int64_t)h * w + (y >> 1) * (w >> 1) + (x >> 1);
    case kYuvYv12: return (int64_t)h * w + plane + (y >> 1) * (w >> 1) + (x >> 1);
    case kYuvUyvy: return yuv_group_offset(layout, h, w, y, x);
    default: return yuv_group_offset(layout, h, w, y, x) + 1;       // P010 (the high byte of the first word), YUYV
  }
}
TSM_HOST_DEVICE inline int64_t yuv_v_offset(int layout, int h, int w, int64_t y, int64_t x) {
  const int64_t plane = (int64_t)(h >> 1) * (w >> 1);
  switch (layout) {
    case kYuvI420: return (int64_t)h * w + plane + (y >> 1) * (w >> 1) + (x >> 1);
    case kYuvYv12: return (int64_t)h * w + (y >> 1) * (w >> 1) + (x >> 1);
    case kYuvUyvy: return yuv_group_offset(layout, h, w, y, x) + 2;
    default: return yuv_group_offset(layout, h, w, y, x) + 3;       // P010 (the high byte of the second word), YUYV
  }
}
// window_descriptor_ok for a window of frames of a YuvLayout: n_segment contiguous frames of yuv_frame_bytes, the sides as
// yuv_sides_ok has them.  (An offset is a multiple of 16 and a frame a multiple of the layout's alignment: every frame of a
// valid window is aligned.)
TSM_HOST_DEVICE inline bool yuv_window_descriptor_ok(int layout, const int32_t d[kWindowDescWords], int n_segment, int64_t arena_bytes,
                                                     bool center, int resize, int crop, int64_t *off, CropGeometry *g) {
  const int64_t o = (int64_t)(((uint64_t)(uint32_t)d[1] << 32) | (uint32_t)d[0]);
  const int h = d[2], w = d[3];
  if (o < 0 || (o & 15) != 0 || h > kWindowMaxSide || w > kWindowMaxSide || !yuv_sides_ok(layout, h, w) || o > arena_bytes) return false;
  int64_t bytes;
  if (__builtin_mul_overflow((int64_t)n_segment, yuv_frame_bytes(layout, h, w), &bytes) || bytes > arena_bytes - o) return false;
  if (center && !center_crop_geometry_int(h, w, resize, crop, g)) return false;
  *off = o;
  return true;
}

// ---- tsm_preprocess_windows in image mode (TSM_WINDOWS_IMAGE): the image model's transform (tsm_preprocess_image: Pillow's
// antialiased 8-bit resample) over windows of different sizes.  Everything the kernel derives from a window's size is here, in
// integers, for the kernel and for the host (tests/image_windows_host.cpp, under ASAN + UBSAN).
// Taps per row of Pillow's coefficient table for one axis: 2 * ceil(max(in / out, 1)) + 1 (pil_ksize of the C ABI, whose
// double quotient has the same ceiling: a non-integral in / out lies at least 1 / out from an integer).  in, out >= 1.
TSM_HOST_DEVICE inline int image_ksize_int(int in, int out) {
  const int64_t c = ((int64_t)in + out - 1) / out;
  return 2 * (int)(c < 1 ? 1 : c) + 1;
}
// LDS rows a band of `band` output rows can need (image_rows_cap's rule, (band - 1) * scale + 2 * support + 2 with scale =
// in / out and support = max(scale, 1), as an exact floor; never below the double's).  1 <= in <= 65535, out >= 1, band <= 8.
TSM_HOST_DEVICE inline int image_rows_cap_int(int band, int in, int out) {
  return in >= out ? (int)(((int64_t)(band + 1) * in) / out) + 2 : (int)(((int64_t)(band - 1) * in) / out) + 4;
}
// Bytes of one LDS row of `crop` pixels (three bytes each, padded to a dword).  crop <= kImageMaxCrop.
constexpr int kImageMaxCrop = 21845;       // the largest crop whose row fits 64 KB
TSM_HOST_DEVICE inline int image_row_stride(int crop) { return (crop * 3 + 3) & ~3; }
// The band of output rows one pass works on: 8, 4, 2 or 1, the largest whose rows fit lds_bytes (`vert`: the height is
// resampled, so a band needs the rows under its vertical support; else its own rows).  0: not even one output row fits.
TSM_HOST_DEVICE inline int image_band(bool vert, int h, int nh, int crop, int lds_bytes, int *rows_cap) {
  for (int band = 8; band >= 1; band /= 2) {
    const int rows = vert ? image_rows_cap_int(band, h, nh) : band;
    if ((int64_t)rows * image_row_stride(crop) <= lds_bytes) {
      *rows_cap = rows;
      return band;
    }
  }
  return 0;
}
// One window of an image-mode launch: d = {off_lo, off_hi, h, w, tab_lo, tab_hi, -, -}; the frames as window_descriptor_ok
// (one byte per channel) or nv12_window_descriptor_ok has them, the centre crop inside the resized frame, and the window's
// coefficient block -- transform.image_tables' layout, [hb crop x 2][hk crop x ksx] when the width changes, then [vb crop x 2]
// [vk crop x ksy] when the height does -- at byte `tab` of the arena: tab >= 0, tab % 16 == 0, tab + 4 * words <= arena_bytes
// (not looked at when the block is empty), and one output row's vertical support within lds_bytes.  True only then, for ANY
// eight int32 words, and no intermediate leaves int64.  n_segment, resize > 0, 0 < crop <= kImageMaxCrop, arena_bytes > 0.
struct ImageWindow {
  int64_t off, tab;            // byte offsets in the arena of the frames and of the table block
  CropGeometry g;
  int ksx, ksy;                // taps per table row; 0: that axis keeps its size and has no table
  int64_t hwords, vwords;      // int32 words of the horizontal and the vertical part of the block
  int band, rows_cap;          // image_band's choice
};
TSM_HOST_DEVICE inline bool image_window_ok(const int32_t d[kWindowDescWords], int n_segment, bool nv12, int64_t arena_bytes, int resize,
                                            int crop, int lds_bytes, ImageWindow *win) {
  if (nv12 ? !nv12_window_descriptor_ok(d, n_segment, arena_bytes, true, resize, crop, &win->off, &win->g)
           : !window_descriptor_ok(d, n_segment, 1, arena_bytes, true, resize, crop, &win->off, &win->g))
    return false;
  const int h = d[2], w = d[3];
  win->ksx = win->g.nw != w ? image_ksize_int(w, win->g.nw) : 0;
  win->ksy = win->g.nh != h ? image_ksize_int(h, win->g.nh) : 0;
  win->hwords = win->ksx ? (int64_t)crop * (2 + win->ksx) : 0;       // < 2^15 * 2^18
  win->vwords = win->ksy ? (int64_t)crop * (2 + win->ksy) : 0;
  const int64_t words = win->hwords + win->vwords;
  win->tab = 0;
  if (words > 0) {
    const int64_t t = (int64_t)(((uint64_t)(uint32_t)d[5] << 32) | (uint32_t)d[4]);
    if (t < 0 || (t & 15) != 0 || t > arena_bytes || 4 * words > arena_bytes - t) return false;
    win->tab = t;
  }
  win->band = image_band(win->ksy != 0, h, win->g.nh, crop, lds_bytes, &win->rows_cap);
  return win->band > 0;
}

// The buffer frames a range of clip windows touches.  Clip c, segment k is source frame step * c + stride * k; a position at or
// past total_frames is the padded tail and reads no video frame; buffer frame j holds source frame stride * (first_frame + j).
// For clips first_clip .. first_clip + n_clips - 1: `tail` = whether any position is padded, `first` = the buffer frame of the
// first position, `last` = that of the last position, or of the video's last frame when the range reaches the tail.
// False -- for ANY arguments, and no intermediate leaves int64 (products of two int32 and their sum only) -- unless the sizes
// are positive, step is a multiple of stride, the first clip starts inside the video and first .. last lie in a buffer of
// n_frames frames.
struct WindowRange {
  int64_t first, last;
  bool tail;
};
inline bool clip_window_range(int64_t total_frames, int64_t first_clip, int n_clips, int n_segment, int step, int stride,
                              int64_t first_frame, int64_t n_frames, WindowRange *r) {
  if (total_frames <= 0 || first_clip < 0 || n_clips <= 0 || n_segment <= 0 || step <= 0 || stride <= 0 || step % stride != 0 ||
      first_frame < 0 || n_frames <= 0)
    return false;
  if (first_clip > (total_frames - 1) / step) return false;       // step * first_clip >= total_frames, without the product
  const int64_t lo = (int64_t)step * first_clip;
  const int64_t span = (int64_t)step * (n_clips - 1) + (int64_t)stride * (n_segment - 1);     // the last position is lo + span
  r->tail = span >= total_frames - lo;
  r->first = lo / stride - first_frame;
  r->last = (r->tail ? total_frames - 1 : lo + span) / stride - first_frame;
  return r->first >= 0 && r->last < n_frames;
}

// ---- ConvNeXt-Base (tsm_set_convnext; timm 0.5.4 convnext_base): the host arithmetic of its schedule ----------------------------
// Four stages of widths 128 / 256 / 512 / 1024; the stem is a 4x4 conv at stride 4, each later stage starts with a 2x2 conv at
// stride 2, both without padding: floor mode, the last h % 4 (h % 2) rows and columns are not read.
constexpr int kCnxStages = 4;
constexpr int kCnxWidths[kCnxStages] = {128, 256, 512, 1024};
constexpr int kCnxMaxDepth = 64;        // blocks per stage an engine accepts (convnext_base: 3, 3, 27, 3)
constexpr float kCnxLnEps = 1e-6f;
constexpr int kCnxStemK = 64;           // the stem as a 1x1 GEMM: K = (ky, kx, c4) = 4 x 4 x 4, channel 3 of every tap zero
// dwconv7_ln_kernel<C>: one lane group per TS x TS output pixels, 4 x 4 but for the last stage's small maps, which take 2 x 2 (tsm_convnext.hip)
TSM_HOST_DEVICE constexpr int cnx_dw_tile(int c) { return c >= 1024 ? 2 : 4; }
inline int cnx_stem_size(int h) { return h > 0 ? h / 4 : 0; }
inline int cnx_down_size(int h) { return h > 0 ? h / 2 : 0; }
// Side of stage s's maps (s in 0 .. 3) for an input side h: ((h / 4) / 2) / 2 ...; 0 when nothing is left.
inline int cnx_stage_size(int h, int s) {
  int v = cnx_stem_size(h);
  for (int i = 0; i < s; ++i) v = cnx_down_size(v);
  return v;
}
// Position of input pixel (y, x)'s channel c in the K axis of the 2x2 space-to-depth row of output pixel (y / 2, x / 2): the
// order (ky, kx, c) of every packed conv weight of the engine (fold_and_pack), ky = y & 1, kx = x & 1.
TSM_HOST_DEVICE inline int64_t cnx_s2d_k(int y, int x, int c, int channels) { return (int64_t)((y & 1) * 2 + (x & 1)) * channels + c; }
// The same for the stem's 4x4 taps over the packed input's 4 channels.
TSM_HOST_DEVICE inline int cnx_stem_k(int ky, int kx, int c) { return (ky * 4 + kx) * 4 + c; }
inline int cnx_tiles_along(int h, int ts) { return (int)(((int64_t)h + ts - 1) / ts); }   // tiles of side ts > 0 that cover a side of h > 0 pixels
// ts x ts output tiles of dwconv7_ln_kernel over n frames of h x w pixels; -1 when the count leaves int32 (its grid) or a size is not positive.
inline int64_t cnx_dw_tiles(int64_t n, int h, int w, int ts) {
  if (n <= 0 || h <= 0 || w <= 0 || ts <= 0) return -1;
  const int64_t ty = cnx_tiles_along(h, ts), tx = cnx_tiles_along(w, ts);
  return mul_sat31(mul_sat31(n, ty), tx) >= kInt31 ? -1 : n * ty * tx;
}
// Floats of the largest activation of one frame: fc1's output in stage 0, 4 * 128 channels on the stem's map (every later
// stage has a quarter of the pixels and twice the channels; the stem's packed patches are 64 wide).  0 when the frame is
// smaller than one stem patch; saturates at 2^31.
inline int64_t cnx_frame_elems(int h, int w) { return mul_sat31(mul_sat31(cnx_stem_size(h), cnx_stem_size(w)), 4 * kCnxWidths[0]); }
// Floats of one workspace buffer for `frames` frames, or -1 when a conv of the schedule could not address it: the conv kernels
// reach their operands through 32-bit byte offsets, so the largest tensor must stay below 2^31 bytes = 2^29 floats.
inline int64_t cnx_workspace_elems(int64_t frames, int h, int w) {
  const int64_t per = cnx_frame_elems(h, w);
  if (frames <= 0 || per <= 0) return -1;
  const int64_t total = mul_sat31(frames, per);
  return total >= (kInt31 >> 2) ? -1 : total;
}
// Why tsm_set_convnext refuses an engine of this shape; nullptr when it can be built.
inline const char *cnx_refusal(int prec, int is_shift, int num_segments, int backbone_set, int non_local, int temporal_pool,
                               const int32_t *depths) {
  if (!depths) return "depths is NULL";
  if (num_segments != 1) return "a ConvNeXt engine is an image model: num_segments must be 1";
  if (is_shift) return "a ConvNeXt engine has no temporal shift: is_shift must be 0";
  if (prec != kPrecF32) return "a ConvNeXt engine runs in TSM_DTYPE_F32 only";
  if (backbone_set) return "tsm_set_convnext excludes tsm_set_backbone / tsm_set_bottleneck_width / tsm_set_shift_place";
  if (non_local) return "tsm_set_convnext excludes tsm_set_non_local";
  if (temporal_pool) return "tsm_set_convnext excludes tsm_set_temporal_pool";
  for (int s = 0; s < kCnxStages; ++s)
    if (depths[s] < 1 || depths[s] > kCnxMaxDepth) return "every stage depth must be in 1 .. 64";
  return nullptr;
}
// Weight packing.  The stem [128, 3, 4, 4] -> [128][64] in cnx_stem_k's order (channel 3 zero); a downsample conv
// [cout, cin, 2, 2] -> [cout][4 cin] in cnx_s2d_k's order; a depthwise conv [c, 1, 7, 7] -> [49][c], tap-major (ky, kx), so
// that the lanes of a pixel read one tap's weights as consecutive 16-byte quads.  All copies, bit for bit.
inline void cnx_pack_stem(const float *w, int cout, std::vector<float> *wp) {
  wp->assign((size_t)cout * kCnxStemK, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < 3; ++c)
      for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx) (*wp)[(size_t)o * kCnxStemK + cnx_stem_k(ky, kx, c)] = w[(((size_t)o * 3 + c) * 4 + ky) * 4 + kx];
}
inline void cnx_pack_down(const float *w, int cout, int cin, std::vector<float> *wp) {
  wp->assign((size_t)cout * 4 * cin, 0.f);
  for (int o = 0; o < cout; ++o)
    for (int c = 0; c < cin; ++c)
      for (int ky = 0; ky < 2; ++ky)
        for (int kx = 0; kx < 2; ++kx) (*wp)[(size_t)o * 4 * cin + (size_t)cnx_s2d_k(ky, kx, c, cin)] = w[(((size_t)o * cin + c) * 2 + ky) * 2 + kx];
}
inline void cnx_pack_dw(const float *w, int c, std::vector<float> *wp) {
  wp->assign((size_t)49 * c, 0.f);
  for (int ch = 0; ch < c; ++ch)
    for (int t = 0; t < 49; ++t) (*wp)[(size_t)t * c + ch] = w[(size_t)ch * 49 + t];
}
// out = x + gamma * (fc2(h) + b) = x + (gamma W) h + gamma b: the layer scale folds into fc2 [c][4 c] as a BatchNorm scale does.
inline void cnx_fold_gamma(const float *w, const float *b, const float *gamma, int cout, int k, std::vector<float> *wp, std::vector<float> *bias) {
  wp->resize((size_t)cout * k);
  bias->resize(cout);
  for (int o = 0; o < cout; ++o) {
    for (int i = 0; i < k; ++i) (*wp)[(size_t)o * k + i] = w[(size_t)o * k + i] * gamma[o];
    (*bias)[o] = b[o] * gamma[o];
  }
}

// ---- TDN-ResNet50 (tsm_set_tdn; include/tsm_hip.h holds the network's definition): the host arithmetic of its schedule --------
constexpr int kTdnFrames = 5;            // frames per segment: 15 input planes
constexpr int kTdnPlanes = 3 * kTdnFrames;
constexpr int kTdnDiffC = 12;            // channels of the stacked frame differences
constexpr int kTdnPatchReal = 7 * 7 * kTdnDiffC;   // 588: conv1_5's K, order (ky, kx, c)
constexpr int kTdnPatchK = 1024;         // ... padded to what conv_igemm's 1x1 form takes: a power-of-two channel count
constexpr int kTdnTile = 8;              // tdn_front_kernel: conv1_5 outputs per workgroup and side
constexpr int kTdnChunkClips = 8;        // clips per front-end chunk through the one patch buffer
constexpr int kTdnMaxDepth = 64;
constexpr int kTdnReduction = 16;        // mSE squeeze: r = C / 16
// torch's 'nearest' source index of output index dst for a side of `in` scaled to `out`: min(int(floorf(dst * ((float)in / out))), in - 1).
TSM_HOST_DEVICE inline int tdn_nearest(int dst, int in, int out) {
  const float scale = (float)in / (float)out;
  const int src = (int)floorf((float)dst * scale);
  return src < in - 1 ? src : in - 1;
}
// Sides along the two paths for an input side h (a multiple of 32, >= 64): the pooled differences h / 2, conv1_5 h / 4, xd0 and
// resnext_layer1 h / 8; the trunk's stem conv h / 2, its max-pool and layer1 h / 4, then h / 8, h / 16, h / 32.
inline int tdn_diff_pool_size(int h) { return h / 2; }
inline int tdn_conv15_size(int h) { return conv_out_size(tdn_diff_pool_size(h), 7, 2); }
inline int tdn_diff_size(int h) { return conv_out_size(tdn_conv15_size(h), 3, 2); }
inline int tdn_stage_size(int h, int layer) {   // layer 1 .. 4: the side of that layer's block outputs
  int v = conv_out_size(conv_out_size(h, 7, 2), 3, 2);
  for (int l = 2; l <= layer; ++l) v = conv_out_size(v, 3, 2);
  return v;
}
inline int tdn_pool_size(int h) { return h / 2; }   // the mSE module's AvgPool2d(2, 2), floor mode
// Why tsm_set_tdn refuses an engine of this shape; nullptr when it can be built.
inline const char *tdn_refusal(int prec, int is_shift, int num_segments, int height, int width, int other_topology, const int32_t *depths) {
  if (!depths) return "depths is NULL";
  if (prec != kPrecF32) return "a TDN engine runs in TSM_DTYPE_F32 only";
  if (is_shift) return "a TDN engine has no TSM shift (its temporal conv is learned): is_shift must be 0";
  if (num_segments < 2) return "a TDN engine needs num_segments >= 2 (the mSE module differences neighbouring segments)";
  if (height < 64 || width < 64 || height % 32 != 0 || width % 32 != 0)
    return "a TDN engine needs height and width that are multiples of 32 and at least 64 (a layer4 mSE map must be poolable)";
  if (other_topology) return "tsm_set_tdn excludes every other tsm_set_* topology call";
  for (int s = 0; s < 4; ++s)
    if (depths[s] < 1 || depths[s] > kTdnMaxDepth) return "every stage depth must be in 1 .. 64";
  return nullptr;
}
// Clips per front-end chunk: at most kTdnChunkClips, and few enough that the patch rows [chunk * T * rows][kTdnPatchK] stay below
// 2^29 floats (the conv kernels' 32-bit byte offsets); 0 when one clip alone does not fit.
inline int tdn_chunk_clips(int max_clips, int T, int h, int w) {
  const int64_t rows = (int64_t)tdn_conv15_size(h) * tdn_conv15_size(w), per_clip = mul_sat31(mul_sat31(rows, T), kTdnPatchK);
  if (per_clip <= 0 || per_clip >= (kInt31 >> 2)) return 0;
  int64_t c = ((kInt31 >> 2) - 1) / per_clip;
  if (c > kTdnChunkClips) c = kTdnChunkClips;
  if (c > max_clips) c = max_clips;
  return (int)c;
}
// K index of tap (ky, kx), difference channel c in a patch row.
TSM_HOST_DEVICE inline int tdn_patch_k(int ky, int kx, int c) { return (ky * 7 + kx) * kTdnDiffC + c; }
// Element of the pooled difference tensor P [hp, wp, 12] that patch-row element k of conv1_5 output (oy, ox) reads: its index, or
// -1 for a padding tap or the K tail (written as zero).
inline int64_t tdn_patch_source(int oy, int ox, int k, int hp, int wp) {
  if (k < 0 || k >= kTdnPatchReal) return -1;
  const int c = k % kTdnDiffC, kx = k / kTdnDiffC % 7, ky = k / kTdnDiffC / 7;
  const int py = 2 * oy - 3 + ky, px = 2 * ox - 3 + kx;
  if (py < 0 || py >= hp || px < 0 || px >= wp) return -1;
  return ((int64_t)py * wp + px) * kTdnDiffC + c;
}
// ---- TSM_LAYOUT_TDN_POOL: where tdn_front_pool_kernel finds the five frames of a segment ----------------------------------------
// Window mode, ONE rule for the kernel and the host: the pool frame of frame j (0 .. 4) of segment k of clip `clip`, or -1 for
// planes of 0.0f.  centre = clip_step * clip + clip_stride * k; the source frame is clamp(centre - 2 + j, 0, total - 1); its pool
// frame is that minus first_source_frame.  A centre >= total, a result outside [0, n_frames) or an argument outside the rule's
// domain takes pad_frame (-1 when that is outside the pool too).  Total in its arguments: no product, sum or difference is formed
// before it is known to fit (tests/tdn_pool_host.cpp runs it at the ends of int64 under UBSAN).
TSM_HOST_DEVICE inline int64_t tdn_window_frame(int64_t first_source_frame, int64_t total_frames, int64_t clip, int k, int j,
                                                int32_t clip_step, int32_t clip_stride, int64_t n_frames, int64_t pad_frame) {
  const int64_t pad = pad_frame >= 0 && pad_frame < n_frames ? pad_frame : -1;
  if (total_frames <= 0 || clip < 0 || k < 0 || j < 0 || j >= kTdnFrames || clip_step <= 0 || clip_stride <= 0) return pad;
  const int64_t last = total_frames - 1;
  int64_t base;
  if (__builtin_mul_overflow((int64_t)clip_step, clip, &base) || base > last) return pad;
  const int64_t off = (int64_t)clip_stride * k;   // (31 + 31 bits)
  if (off > last - base) return pad;              // the centre is past the end
  const int64_t centre = base + off;
  const int d = j - 2;
  const int64_t src = d > 0 ? (d > last - centre ? last : centre + d) : (centre < -d ? 0 : centre + d);
  if (src < first_source_frame) return pad;
  if (first_source_frame < 0 && src > INT64_MAX + first_source_frame) return pad;   // (src - first would not fit: far outside any pool)
  const int64_t rel = src - first_source_frame;
  return rel < n_frames ? rel : pad;
}
// A table entry: range-tested in 32 bits first, only then widened.  `limit` = tdn_table_limit(n_frames).
TSM_HOST_DEVICE inline int64_t tdn_table_frame(int32_t entry, uint32_t limit) { return (uint32_t)entry < limit ? (int64_t)entry : -1; }
inline uint32_t tdn_table_limit(int64_t n_frames) { return n_frames <= 0 ? 0u : n_frames > (int64_t)INT32_MAX ? 0x80000000u : (uint32_t)n_frames; }
// What tdn_front_pool_kernel takes by value: a tsm_tdn_pool behind its checks, the table / first clip advanced to the launch's first
// segment.  Nothing in it points to host memory.
struct TdnPoolSource {
  const float *frames;
  const int32_t *index;   // mode 0, else nullptr
  int64_t n_frames, first_source_frame, total_frames, first_clip, pad_frame;
  int32_t clip_step, clip_stride, mode, T;
  uint32_t limit;         // tdn_table_limit(n_frames)
};
// Why a forward refuses this descriptor (TSM_ERR_INVALID_ARG); nullptr when it can run.
inline const char *tdn_pool_refusal(const tsm_tdn_pool *d) {
  if (!d) return "clips is NULL";
  if (d->struct_size != sizeof(tsm_tdn_pool)) return "tsm_tdn_pool: struct_size is not sizeof(tsm_tdn_pool)";
  if (d->mode != 0 && d->mode != 1) return "tsm_tdn_pool: mode must be 0 (table) or 1 (window)";
  if (!d->frames) return "tsm_tdn_pool: frames is NULL";
  if (reinterpret_cast<uintptr_t>(d->frames) % 8 != 0) return "tsm_tdn_pool: frames must be 8-byte aligned";
  if (d->n_frames <= 0) return "tsm_tdn_pool: n_frames must be positive";
  if (d->mode == 0 && !d->index) return "tsm_tdn_pool: table mode needs index";
  if (d->mode == 1 && (d->clip_step <= 0 || d->clip_stride <= 0)) return "tsm_tdn_pool: clip_step and clip_stride must be positive";
  if (d->mode == 1 && d->total_frames <= 0) return "tsm_tdn_pool: total_frames must be positive";
  return nullptr;
}
// The descriptor as the kernel's parameter, for the chunk that starts `clip0` clips into the call.
inline TdnPoolSource tdn_pool_source(const tsm_tdn_pool &d, int T, int64_t clip0) {
  TdnPoolSource p{};
  p.frames = d.frames;
  p.n_frames = d.n_frames;
  p.mode = d.mode;
  p.T = T;
  p.limit = tdn_table_limit(d.n_frames);
  p.pad_frame = -1;
  if (d.mode == 0) {
    p.index = d.index + clip0 * T * kTdnFrames;
  } else {
    p.first_source_frame = d.first_source_frame;
    p.total_frames = d.total_frames;
    p.first_clip = d.first_clip > INT64_MAX - clip0 ? INT64_MAX : d.first_clip + clip0;   // (saturated: past every video's end)
    p.clip_step = d.clip_step;
    p.clip_stride = d.clip_stride;
    p.pad_frame = d.pad_frame;
  }
  return p;
}
// ---- The forward in two phases (TSM_LAYOUT_TDN_SEGMENTS / TSM_LAYOUT_TDN_RING) ------------------------------------------------
// A segment descriptor's frame fields as the tsm_tdn_pool a front-end launch reads: a segment is a clip of ONE segment, so the
// window rule runs with T = 1 and clip_step = clip_stride (centre = clip_stride * (first_clip + i)).
inline tsm_tdn_pool tdn_segments_pool(const tsm_tdn_segments &d) {
  tsm_tdn_pool p{};
  p.struct_size = sizeof(tsm_tdn_pool);
  p.mode = d.mode;
  p.frames = d.frames;
  p.n_frames = d.n_frames;
  p.index = d.index;
  p.first_source_frame = d.first_source_frame;
  p.total_frames = d.total_frames;
  p.first_clip = d.first_clip;
  p.clip_step = d.clip_stride;
  p.clip_stride = d.clip_stride;
  p.pad_frame = d.pad_frame;
  return p;
}
// Why a segment-phase call refuses this descriptor (TSM_ERR_INVALID_ARG); nullptr when it can run.
inline const char *tdn_segments_refusal(const tsm_tdn_segments *d) {
  if (!d) return "clips is NULL";
  if (d->struct_size != sizeof(tsm_tdn_segments)) return "tsm_tdn_segments: struct_size is not sizeof(tsm_tdn_segments)";
  if (d->mode != 0 && d->mode != 1) return "tsm_tdn_segments: mode must be 0 (table) or 1 (window)";
  if (!d->frames) return "tsm_tdn_segments: frames is NULL";
  if (reinterpret_cast<uintptr_t>(d->frames) % 8 != 0) return "tsm_tdn_segments: frames must be 8-byte aligned";
  if (d->n_frames <= 0) return "tsm_tdn_segments: n_frames must be positive";
  if (d->mode == 0 && !d->index) return "tsm_tdn_segments: table mode needs index";
  if (d->mode == 0 && reinterpret_cast<uintptr_t>(d->index) % 4 != 0) return "tsm_tdn_segments: index must be 4-byte aligned";
  if (d->mode == 1 && d->clip_stride <= 0) return "tsm_tdn_segments: clip_stride must be positive";
  if (d->mode == 1 && d->total_frames <= 0) return "tsm_tdn_segments: total_frames must be positive";
  if (!d->out_a || !d->out_d) return "tsm_tdn_segments: out_a / out_d is NULL";
  if (reinterpret_cast<uintptr_t>(d->out_a) % 16 != 0 || reinterpret_cast<uintptr_t>(d->out_d) % 16 != 0)
    return "tsm_tdn_segments: out_a and out_d must be 16-byte aligned";
  return nullptr;
}
// Why a trunk-phase call refuses this descriptor (TSM_ERR_INVALID_ARG); nullptr when it can run.
inline const char *tdn_ring_refusal(const tsm_tdn_ring *d) {
  if (!d) return "clips is NULL";
  if (d->struct_size != sizeof(tsm_tdn_ring)) return "tsm_tdn_ring: struct_size is not sizeof(tsm_tdn_ring)";
  if (d->n_slots <= 0) return "tsm_tdn_ring: n_slots must be positive";
  if (!d->ring_a || !d->ring_d) return "tsm_tdn_ring: ring_a / ring_d is NULL";
  if (reinterpret_cast<uintptr_t>(d->ring_a) % 16 != 0 || reinterpret_cast<uintptr_t>(d->ring_d) % 16 != 0)
    return "tsm_tdn_ring: ring_a and ring_d must be 16-byte aligned";
  if (!d->table) return "tsm_tdn_ring: table is NULL";
  if (reinterpret_cast<uintptr_t>(d->table) % 4 != 0) return "tsm_tdn_ring: table must be 4-byte aligned";
  return nullptr;
}
// The slot rule, ONE for the kernel and the host: a table entry's ring slot, or -1 for "no segment: zeros".  Range-tested in 32
// bits, only then widened (total in the entry: INT32_MIN and INT32_MAX are -1 unless inside the ring).
TSM_HOST_DEVICE inline int64_t tdn_ring_slot(int32_t entry, int32_t n_slots) {
  return n_slots > 0 && (uint32_t)entry < (uint32_t)n_slots ? (int64_t)entry : -1;
}
// Which side of the seam a tap name lies on: true for the stages the segment phase computes ("diff.*", "stem", "fuse1",
// "resnext_layer1.*", "layer1.*"), false for "fuse2" and everything behind it (and any unknown name: the trunk phase reports it).
inline bool tdn_stage_in_segment_phase(const char *stage) {
  if (!stage) return false;
  const std::string s(stage);
  auto starts = [&](const char *p) { return s.compare(0, strlen(p), p) == 0; };
  return s == "stem" || s == "fuse1" || starts("diff.") || starts("resnext_layer1.") || starts("layer1.");
}
// Tile-cache keys: a whole forward's bucket is its frame count bucket(n_clips) * T; the phases keep vectors of their own (each
// tunes only its own convs), keyed by the frame count of the bucket plus a phase tag no whole forward's frame count reaches.
constexpr int kTdnSegmentsKey = 1 << 28, kTdnRingKey = 1 << 29;

// conv1_5 [64, 12, 7, 7] + its BatchNorm -> [64][kTdnPatchK] in tdn_patch_k's order, the K tail zero.
inline void tdn_pack_conv15(const float *w, const float *gamma, const float *beta, const float *mean, const float *var, int cout,
                            std::vector<float> *wp, std::vector<float> *bias) {
  wp->assign((size_t)cout * kTdnPatchK, 0.f);
  bias->resize(cout);
  for (int o = 0; o < cout; ++o) {
    const float scale = gamma[o] / std::sqrt(var[o] + kBnEps);
    (*bias)[o] = beta[o] - mean[o] * scale;
    for (int c = 0; c < kTdnDiffC; ++c)
      for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx)
          (*wp)[(size_t)o * kTdnPatchK + tdn_patch_k(ky, kx, c)] = w[(((size_t)o * kTdnDiffC + c) * 7 + ky) * 7 + kx] * scale;
  }
}
// A conv bias in front of a BatchNorm: BN(conv(x) + b) = conv(x) * s + (beta + (b - mean) * s), i.e. the same BatchNorm with the
// running mean moved by b.  Returns mean - b, which the bias-free folds (fold_and_pack, the stem's) then take as their mean.
inline std::vector<float> tdn_mean_less_bias(const float *mean, const float *cbias, int cout) {
  std::vector<float> m(cout);
  for (int o = 0; o < cout; ++o) m[o] = mean[o] - cbias[o];
  return m;
}
// The mSE module's weights as its kernels read them (tsm_tdn.hip), every BatchNorm folded into a scale on the weights and a bias.
//   squeeze  mse.conv1 [r, C, 1, 1] + bn1          -> wq [C][r] (output channel fastest), bq [r]
//   dw       mse.conv2 [r, 1, 3, 3]                -> [9][r], tap-major (ky, kx)
//   k2 / k4  mse.conv3_smallscale{2,4} [r, r, 3, 3] + their bn -> [9][r in][r out], bias [r]
//   excite   mse.conv3 [C, r, 1, 1] + bn3          -> [C][r], bias [C]
//   temporal shift.conv.weight [C, 1, 3]           -> [3][C], tap-major
struct TdnMseWeights {
  std::vector<float> wq, bq, dw, k2, b2, k4, b4, w3, b3, wt;
};
inline void tdn_bn_fold(const float *bn, int c, std::vector<float> *scale, std::vector<float> *bias) {   // bn = [gamma | beta | mean | var], c each
  scale->resize(c);
  bias->resize(c);
  for (int o = 0; o < c; ++o) {
    (*scale)[o] = bn[o] / std::sqrt(bn[3 * (size_t)c + o] + kBnEps);
    (*bias)[o] = bn[(size_t)c + o] - bn[2 * (size_t)c + o] * (*scale)[o];
  }
}
inline void tdn_pack_mse(int C, const float *conv1, const float *bn1, const float *conv2, const float *k2, const float *bn2, const float *k4,
                         const float *bn4, const float *conv3, const float *bn3, const float *shift_w, TdnMseWeights *out) {
  const int r = C / kTdnReduction;
  std::vector<float> s;
  tdn_bn_fold(bn1, r, &s, &out->bq);
  out->wq.assign((size_t)C * r, 0.f);
  for (int j = 0; j < r; ++j)
    for (int c = 0; c < C; ++c) out->wq[(size_t)c * r + j] = conv1[(size_t)j * C + c] * s[j];
  out->dw.assign((size_t)9 * r, 0.f);
  for (int j = 0; j < r; ++j)
    for (int t = 0; t < 9; ++t) out->dw[(size_t)t * r + j] = conv2[(size_t)j * 9 + t];
  for (int which = 0; which < 2; ++which) {
    const float *k = which ? k4 : k2;
    std::vector<float> &kp = which ? out->k4 : out->k2;
    tdn_bn_fold(which ? bn4 : bn2, r, &s, which ? &out->b4 : &out->b2);
    kp.assign((size_t)9 * r * r, 0.f);
    for (int j = 0; j < r; ++j)
      for (int i = 0; i < r; ++i)
        for (int t = 0; t < 9; ++t) kp[((size_t)t * r + i) * r + j] = k[((size_t)j * r + i) * 9 + t] * s[j];
  }
  tdn_bn_fold(bn3, C, &s, &out->b3);
  out->w3.assign((size_t)C * r, 0.f);
  for (int c = 0; c < C; ++c)
    for (int i = 0; i < r; ++i) out->w3[(size_t)c * r + i] = conv3[(size_t)c * r + i] * s[c];
  out->wt.assign((size_t)3 * C, 0.f);
  for (int c = 0; c < C; ++c)
    for (int t = 0; t < 3; ++t) out->wt[(size_t)t * C + c] = shift_w[(size_t)c * 3 + t];
}

// Tuned tile shapes are cached per power-of-two bucket of the clip count (ragged last batches of a video
// would otherwise each pay a tuning pass): the first clip count that lands in a bucket tunes it.
inline int tile_bucket(int n_clips) {
  int b = 1;
  while (b < n_clips) b <<= 1;
  return b;
}


// conv3 weights of a fused conv2+conv3 block (conv23_fused_kernel / conv23_fused2_kernel) in MFMA-fragment order.  w3p is
// the packed, BN-folded matrix [nchunk * cmid][cmid] (nchunk = 4, or 2 for the Cout = 2 * cmid form); the kernel's wave
// `wn` (of cmid / 32) loads, for output chunk j (of nchunk, cmid channels each) and k-group kk (of cmid / 8), ONE 16-byte
// element per lane:
//   out[(((j * wgn + wn) * nkk + kk) * 64 + lane) * 4 + s] = W3[n = j * cmid + wn * 32 + (lane & 31)][k = 8 kk + 4 (lane >> 5) + s]
// i.e. exactly the B operand of v_mfma_f32_32x32x2_f32 step s of that k-group, so the load is lane-linear (coalesced).
inline void pack_w3_fragments(const float *w3p, int cmid, std::vector<float> *out, int nchunk = 4) {
  const int wgn = cmid / 32, nkk = cmid / 8;
  out->assign((size_t)nchunk * cmid * cmid, 0.f);
  for (int j = 0; j < nchunk; ++j)
    for (int wn = 0; wn < wgn; ++wn)
      for (int kk = 0; kk < nkk; ++kk)
        for (int lane = 0; lane < 64; ++lane)
          for (int s = 0; s < 4; ++s) {
            const int n = j * cmid + wn * 32 + (lane & 31), k = 8 * kk + 4 * (lane >> 5) + s;
            (*out)[((((size_t)j * wgn + wn) * nkk + kk) * 64 + lane) * 4 + s] = w3p[(size_t)n * cmid + k];
          }
}

// The same for a split-bf16 engine: per output chunk j, wave wn and k16 group kq the kernel loads TWO 16-byte elements
// per lane, the hi and the lo halves of the 8 channels k = 16 kq + 8 (lane >> 5) + 0..7 of row n:
//   element (((j * wgn + wn) * (2 * nkq) + 2 * kq + part) * 64 + lane), part 0 = hi x8, 1 = lo x8  (bf16 pairs per float slot)
// with hi = bf16(w), lo = bf16(w - hi) exactly as to_split() stores the conv3 weights of the un-fused path.
inline void pack_w3_fragments_split(const float *w3p, int cmid, std::vector<float> *out, int nchunk = 4) {
  const int wgn = cmid / 32, nkq = cmid / 16;
  out->assign((size_t)nchunk * cmid * cmid, 0.f);
  uint16_t *o = reinterpret_cast<uint16_t *>(out->data());
  for (int j = 0; j < nchunk; ++j)
    for (int wn = 0; wn < wgn; ++wn)
      for (int kq = 0; kq < nkq; ++kq)
        for (int lane = 0; lane < 64; ++lane) {
          const int n = j * cmid + wn * 32 + (lane & 31), k0 = 16 * kq + 8 * (lane >> 5);
          const size_t base = ((((size_t)j * wgn + wn) * (2 * nkq) + 2 * kq) * 64 + lane) * 8;   // in bf16 units
          for (int e = 0; e < 8; ++e) {
            const float x = w3p[(size_t)n * cmid + k0 + e];
            const uint16_t hi = f2bf(x);
            o[base + e] = hi;
            o[base + 64 * 8 + e] = f2bf(x - bf2f(hi));
          }
        }
}

// A layer's tile code (TSM_TUNE_CACHE lines, tsm_conv_tiles): a ConvTile in the low bits, plus flags.  The fusion bits sit on the
// code of the first conv they replace and say that the fused form was chosen; it runs only where it can (tsm_engine.hip,
// plan_forward).
constexpr int kCodeTileMask = 0xF;     // the ConvTile
constexpr int kCodePosMajor = 0x80;    // position-major rows of a segmented fp32 3x3 on 64x64 tiles (ConvParams::pos_major), alone or with kCodeTailK
constexpr int kCodeSplitK = 0x100;     // split-K form of a segmented fp32 layer
constexpr int kCodeTailK = 0x200;      // tail split of a segmented 64x64 layer (ConvParams::ksplit = 2)
constexpr int kCodeConv23 = 0x400;     // on conv2: conv2 + conv3 + residual as one launch
constexpr int kCodeBlock = 0x800;      // on conv1: the whole Bottleneck as one launch
constexpr int kCodeConv31 = 0x1000;    // on conv3: conv3 + the next block's shift + conv1 as one launch
constexpr int kCodeFront = 0x2000;     // on conv1: shift + conv1 + the block's stride-2 conv2 as one launch
constexpr int kCodeFused = kCodeConv23 | kCodeBlock | kCodeConv31 | kCodeFront;
constexpr int kCodeValid = kCodeTileMask | kCodePosMajor | kCodeSplitK | kCodeTailK | kCodeFused;   // every bit a code may carry
static_assert((kCodeOpSegmented & kCodeValid) == 0, "the per-op segmented bit must stay clear of the engine's code bits");

// One line of a TSM_TUNE_CACHE file: "<signature>|<bucket>|c0,c1,...".  Succeeds only when the line starts with
// `want`, holds exactly codes->size() integers and each is a ConvTile below `num_tiles` with no bit outside kCodeValid.
// Anything else (foreign keys, truncated lines, garbage, overlong numbers) leaves *codes untouched.
inline bool parse_tune_line(const char *line, const std::string &want, int num_tiles, std::vector<int> *codes) {
  if (strncmp(line, want.c_str(), want.size()) != 0) return false;
  std::vector<int> got;
  const char *q = line + want.size();
  while (*q && *q != '\n') {
    char *end = nullptr;
    const long v = strtol(q, &end, 10);
    if (end == q) return false;
    if (v < 0 || (v & ~(long)kCodeValid) != 0 || (int)(v & kCodeTileMask) >= num_tiles) return false;
    got.push_back((int)v);
    if (*end == ',') q = end + 1;
    else if (*end == '\n' || *end == 0) q = end;
    else return false;
  }
  if (got.size() != codes->size()) return false;
  *codes = got;
  return true;
}

}  // namespace tsm_host
