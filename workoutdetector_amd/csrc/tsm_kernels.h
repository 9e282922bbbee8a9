// Internal launch API shared by the kernel files (csrc/tsm_*.hip, device code; tsm_device.h lists them) and tsm_engine.hip (host engine).
// gfx950 only.  All activations NHWC fp32; weights packed [Cout][Kp] with K = (ky, kx, c).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// The parameter blocks, tile codes and every launch rule (conv_route, conv_tile_valid, the fused forms' *_valid): HIP-free.
#include "tsm_conv_rules.h"

namespace tsm_host {
struct TdnPoolSource;   // tsm_host_util.h: tdn_front_pool_kernel's parameter
}

namespace tsm {

// ks in {1, 3, 7}.  conv_route (tsm_conv_rules.h) decides; returns hipSuccess, hipErrorInvalidValue for a refused route, or the launch error.
hipError_t launch_conv(const ConvParams &p, int ks, hipStream_t s);
// Fused23Params: cout3 = conv3's output channels: 4 * cmid (conv23_fused_kernel), or 2 * cmid with cmid = 128 (conv23_fused2_kernel)
hipError_t launch_conv23_fused(const Fused23Params &p, int cmid, int cout3, int prec, hipStream_t s);
hipError_t launch_bneck_ws(const BneckParams &p, hipStream_t s);
hipError_t launch_front_s2(const FrontParams &p, hipStream_t s);
hipError_t launch_conv31_fused(const Conv31Params &p, hipStream_t s);

// Stem (7x7 s2 p3, 3 -> 64) of the bf16 formats as a direct convolution from an LDS-resident pixel-pair patch; x is the
// packed-pair input [n][hi][ceil(wi/2)][8], w the engine's packed stem weights [64][kp], y NHWC, all in `prec`'s format
// (kPrecBf16 or kPrecBf16x3).  Bit-identical to launch_conv(ks = 7) on the same operands.
hipError_t launch_stem_direct(const float *x, const float *w, const float *bias, float *y, int n, int hi, int wi, int kp,
                              int relu, int prec, hipStream_t s);
// The same stem with the 3x3 stride-2 max-pool fused behind it: y is the POOLED tensor [n][hp][wp][64]; the stem's own
// output is never materialised.  Bit-identical to launch_stem_direct followed by launch_maxpool3x3s2.
// planar != 0: x is the [n][3][hi][wi] fp32 tensor (the reference model's input) and the kernel converts it the way
// launch_pack_input would have -- the same bits without the pack launch and its packed copy.
hipError_t launch_stem_pool(const float *x, const float *w, const float *bias, float *y, int n, int hi, int wi, int kp,
                            int relu, int prec, hipStream_t s, int planar = 0);
// y = act(((p[0] + p[1]) + ...) + bias (+ res)) over fp32 partial tiles [n_seg][M*Cout] written by a ksplit launch.
hipError_t launch_splitk_reduce(const float *partial, int n_seg, int64_t m, int cout, const float *bias,
                                const float *res, float *y, int relu, hipStream_t s);
// The tail of a position-major launch (ConvParams::pos_major): partial is [n_seg][m rows][cout] for the GEMM rows m_first ..
// m_first + m - 1 = n_frames * howo - 1; row m' goes to row (m' % n_frames) * howo + m' / n_frames of y, the WHOLE output.
hipError_t launch_splitk_reduce_pos(const float *partial, int n_seg, int64_t m_first, int64_t m, int n_frames, int howo, int cout,
                                    const float *bias, float *y, int relu, hipStream_t s);

// prec == kPrecF32: dst is NHWC4 fp32; bf16 formats: one 8-element group per pixel PAIR (rows of ceil(w/2) groups).
hipError_t launch_pack_input(const float *src, float *dst, int64_t n_frames, int h, int w,
                             int nchw, int prec, hipStream_t s);
// fp32 [n8 * 8 channels] <-> the storage format of `prec` (kPrecBf16x3 or kPrecBf16)
hipError_t launch_from_f32(const float *x, float *y, int64_t n8, int prec, hipStream_t s);
hipError_t launch_to_f32(const float *x, float *y, int64_t n8, int prec, hipStream_t s);
// Fused test transform: [n,h,w,3] u8|f32 (or [n,3h/2,w] NV12) frames -> resize (short side -> `resize`, bilinear, no
// antialias, align_corners=False) -> centre crop -> ImageNet normalise -> NHWC4 (out_nchw=0) or NCHW.
struct PreprocParams {
  const void *src;
  float *dst;
  int n, h, w;        // source frames
  int nh, nw;         // resized size
  int top, left, crop;
  int src_is_u8;
  int src_yuv;        // 0: RGB frames; 1: NV12; 2 + tsm_host::YuvLayout: I420 .. UYVY.  Converted in the taps; src_is_u8 is 0
  int32_t nv12[6];    // tsm_host::Nv12Coef's words {y_off, cy, crv, cgu, cgv, cbu} (tsm_host_util.h)
  int out_mode;       // 0 = NHWC4 fp32, 1 = NCHW fp32, 2 = NHWC8 split-bf16, 3 = NHWC8 bf16
  float pre_scale;    // 1/255 when frames are to be scaled to [0,1] first, else 1
};
hipError_t launch_preprocess(const PreprocParams &p, hipStream_t s);

// Clips out of a buffer of transformed frames (see gather_clips_kernel).  Buffer frame j holds source frame
// clip_stride * (first_frame + j); pad_frame is the buffer's frame for positions past the end of the video.
struct GatherParams {
  const void *frames;
  void *out;
  int64_t n_frames, frame_bytes, first_frame, total_frames, first_clip, pad_frame;
  int n_clips, n_segment, clip_step, clip_stride;
  int64_t row0;   // first (clip, segment) row of this launch (set by launch_gather_clips: one launch cuts <= 65535 rows)
};
hipError_t launch_gather_clips(const GatherParams &p, hipStream_t s);

// Person-crop test transform fused with the clip iterator (see preprocess_clips_kernel): staged raw frames [n_frames,h,w,3]
// u8|f32 (buffer frame j = source frame clip_stride * (first_frame + j), as GatherParams) + one box per clip -> out
// [n_clips, n_segment, ...one frame of `size`] in any out_mode of PreprocParams.  The launcher validates every FRAME index on
// the host (hipErrorInvalidValue, nothing launched); the kernel is total in the BOX contents, which live in device memory.
struct ClipPreprocParams {
  const void *src;
  float *dst;
  const int *boxes;   // device, [n_clips, 4] = (top, left, bh, bw) in source-frame pixels; bh <= 0 or bw <= 0: the whole frame
  int64_t n_frames, first_frame, total_frames, first_clip;
  int n_clips, n_segment, clip_step, clip_stride;
  int h, w, size;
  int src_is_u8;
  int src_yuv;        // 0: RGB frames; 1: NV12; 2 + tsm_host::YuvLayout: I420 .. UYVY.  Converted in the taps; src_is_u8 is 0
  int32_t nv12[6];    // tsm_host::Nv12Coef's words {y_off, cy, crv, cgu, cgv, cbu} (tsm_host_util.h)
  int out_mode;       // as PreprocParams
  float pre_scale;
};
hipError_t launch_preprocess_clips(const ClipPreprocParams &p, hipStream_t s);

// The centre-crop test transform through a device index table (see preprocess_indexed_kernel): staged raw frames
// [n_frames,h,w,3] u8|f32 -> out row r = launch_preprocess' result for buffer frame index[r], r < n_rows = n_clips * n_segment,
// in any out_mode.  `pp` is launch_preprocess' geometry (pp.n is not used); the kernel is total in the TABLE contents, which
// live in device memory: an entry outside [0, n_frames) reads nothing and yields the normalised zero frame.
struct IndexedPreprocParams {
  PreprocParams pp;
  const int *index;   // device, [n_rows] buffer-frame numbers
  int64_t n_frames, n_rows;
};
hipError_t launch_preprocess_indexed(const IndexedPreprocParams &p, hipStream_t s);

// Either test transform over windows of DIFFERENT frame sizes (see preprocess_windows_kernel): window c is n_segment
// contiguous raw frames [h, w, 3] u8|f32 somewhere in one device arena, described by 8 int32 words of a device table
// (tsm_host::window_descriptor_ok) -> out [n_windows, n_segment, ...one frame of `crop`] in any out_mode.  person_crop 0:
// launch_preprocess' transform with the geometry of each window's own size; 1: launch_preprocess_clips' with the window's box.
// The kernel is total in the TABLE contents, which live in device memory: an invalid descriptor reads nothing and yields
// the normalised zero frame for every row of its window.
struct WindowPreprocParams {
  const void *arena;
  float *dst;
  const int *desc;    // device, 16-byte aligned, [n_windows, 8] = {off_lo, off_hi, h, w, top, left, bh, bw}
  int64_t arena_bytes;
  int n_windows, n_segment;
  int person_crop;
  int resize, crop;   // crop: the output size in both modes
  int src_is_u8;
  int src_yuv;        // 0: RGB frames; 1: NV12; 2 + tsm_host::YuvLayout: I420 .. UYVY.  Converted in the taps; src_is_u8 is 0
  int32_t nv12[6];    // tsm_host::Nv12Coef's words {y_off, cy, crv, cgu, cgv, cbu} (tsm_host_util.h)
  int out_mode;       // as PreprocParams
  float pre_scale;
};
hipError_t launch_preprocess_windows(const WindowPreprocParams &p, hipStream_t s);

// The image model's per-frame transform (see preprocess_image_kernel): staged uint8 frames [n,h,w,3] -> Pillow's antialiased
// bilinear resize to nh x nw (integer arithmetic from host-built tables), the crop window (top, left, crop) of it, normalised
// and packed in any out_mode of PreprocParams.  Tables (device int32, rows for the crop window's output indices only):
// hb / vb [crop][2] = (first source index, taps), hk / vk [crop][ksx | ksy] = weights scaled by 2^22; hk == nullptr or
// vk == nullptr skips that pass (legal only where the axis keeps its size).  The launcher picks band / rows_cap / stride and
// returns hipErrorNotSupported when one output row's vertical support does not fit kImageMaxLds.
constexpr int kImageMaxLds = 65536;
struct ImagePreprocParams {
  const unsigned char *src;
  float *dst;
  const int *hb, *hk, *vb, *vk;
  int n, h, w;        // source frames
  int nh, nw;         // resized size
  int top, left, crop;
  int ksx, ksy;       // taps per table row
  int out_mode;       // as PreprocParams
  int band, rows_cap, stride;   // set by the launcher: output rows per workgroup, LDS rows, bytes per LDS row
};
hipError_t launch_preprocess_image(ImagePreprocParams p, hipStream_t s);
// launch_preprocess_image's transform over windows of different sizes (see preprocess_image_windows_kernel): p.desc rows are
// {off_lo, off_hi, h, w, tab_lo, tab_hi, -, -} (tsm_host::image_window_ok), frames uint8 RGB (src_is_u8) or NV12 (src_yuv 1),
// person_crop and pre_scale are not read.  One launch with kImageMaxLds of dynamic LDS; hipErrorNotSupported for any other
// frame format or a crop beyond tsm_host::kImageMaxCrop.
hipError_t launch_preprocess_image_windows(const WindowPreprocParams &p, hipStream_t s);

// The image model's vote (see frame_votes_kernel): pred [n] = first arg-max, state [n] = (sum of the last <= 7 preds) >= 4,
// hist_in [n_hist <= 6] the preds before this batch (oldest first), hist_out [6] (nullable, must not alias hist_in) the last
// min(6, n_hist + n) afterwards.
hipError_t launch_frame_votes(const float *logits, int n, int c, const int *hist_in, int n_hist, int *pred, int *state,
                              int *hist_out, hipStream_t s);

// Accuracy tally (see top1_tally_kernel): pred [n] (nullable) = first arg-max of logits [n, c]; for a label in [0, c):
// total[label] += 1, correct[label] += (pred == label); any other label is counted nowhere.  correct / total [c] ACCUMULATE.
// c <= kTallyMaxClass, else hipErrorNotSupported.
constexpr int kTallyMaxClass = 1024;
hipError_t launch_top1_tally(const float *logits, const int *labels, int n, int c, int *pred, int *correct, int *total,
                             hipStream_t s);

hipError_t launch_maxpool3x3s2(const float *x, float *y, int n, int hi, int wi, int c, int prec,
                               hipStream_t s);
hipError_t launch_temporal_shift(const float *x, float *y, int64_t n_frames, int n_segment,
                                 int64_t hw, int c, int fold, hipStream_t s);
// temporal max-pool (see temporal_maxpool_kernel): x [n_clips * T, hw, c] -> y [n_clips * T / 2, hw, c] in `prec`'s storage
// format (kPrecF32 or kPrecBf16x3), kernel 3 / stride 2 / padding 1 over the frames of each clip; T even, c a multiple of the
// format's channel group; anything else hipErrorInvalidValue, nothing launched
hipError_t launch_temporal_maxpool(const float *x, float *y, int64_t n_clips, int T, int64_t hw, int c, int prec, hipStream_t s);
// pooled: scratch [n_clips * n_segment, c]
hipError_t launch_head(const float *feat, const float *fc_w, const float *fc_b, float *pooled,
                       float *logits, int n_clips, int n_segment, int hw, int c, int num_class, int prec,
                       hipStream_t s);
// per-segment head: logits [n_frames, num_class], one launch, no scratch (c % 8 == 0, c <= 2048)
hipError_t launch_head_segments(const float *feat, const float *fc_w, const float *fc_b, float *logits, int n_frames,
                                int hw, int c, int num_class, int prec, hipStream_t s);
// frame embeddings (see pool_feat_kernel): pooled / unit [n_frames, c], either nullable; one launch (c % 8 == 0, c <= 2048)
hipError_t launch_pool_features(const float *feat, float *pooled, float *unit, int n_frames, int hw, int c, int prec,
                                hipStream_t s);
// cosine-distance band (see cosine_dist_kernel, tsm_similarity.hip): rows [row0, row1) x columns [0, row1) of dist
// [n_total, n_total] and their mirror, from unit rows [n_total, c] (c % 8 == 0)
hipError_t launch_cosine_distances(const float *unit, int n_total, int c, int row0, int row1, float *dist, hipStream_t s);

// non-local block (tsm_nonlocal.hip).  maxpool2x2: 2x2 / stride 2 / floor-mode max-pool of channels [c0, c0 + c) of NHWC rows
// `ld` floats apart into the dense [n, hi / 2, wi / 2, c] tensor y (c0, c, ld multiples of 4; hi, wi >= 2).
hipError_t launch_maxpool2x2(const float *x, int64_t ld, int c0, int c, float *y, int n, int hi, int wi, hipStream_t s);
// y[b, i, :] = sum_j softmax_j(q[b, i, :] . k[b, j, :]) v[b, j, :] (see nonlocal_attn_kernel): rows of q / k, v / y are ldq / ldkv /
// ldy floats apart (ldq, ldkv multiples of 4; q, k, v 16-byte aligned).  d in {256, 512}, else hipErrorNotSupported (nothing launched).
hipError_t launch_nonlocal_attention(const float *q, int64_t ldq, const float *k, const float *v, int64_t ldkv, float *y,
                                     int64_t ldy, int n_clips, int nq, int nk, int d, hipStream_t s);

// ConvNeXt-Base (tsm_convnext.hip), fp32 NHWC, c in {128, 256, 512, 1024}; anything else hipErrorInvalidValue, nothing launched.
// dwconv7_ln: y = LayerNorm_c(depthwise 7x7 (padding 3) of x + b) on [n, h, w, c]; w [49][c] (tsm_host::cnx_pack_dw).
hipError_t launch_dwconv7_ln(const float *x, const float *w, const float *b, const float *ln_w, const float *ln_b, float *y, int n,
                             int h, int wi, int c, hipStream_t s);
// LayerNorm over the c channels of every row of x [rows][c] (biased variance, eps 1e-6, affine)
hipError_t launch_layer_norm(const float *x, const float *ln_w, const float *ln_b, float *y, int64_t rows, int c, hipStream_t s);
// the same per pixel of x [n, h, w, c], written as 2x2 space-to-depth rows y [n, h / 2, w / 2, 4 c] (K order: tsm_host::cnx_s2d_k)
hipError_t launch_layer_norm_s2d(const float *x, const float *ln_w, const float *ln_b, float *y, int n, int h, int w, int c, hipStream_t s);
// the packed fp32 input [n, h, w, 4] -> the stem's 4x4 patches [n, h / 4, w / 4, 64] (K order: tsm_host::cnx_stem_k)
hipError_t launch_stem_pack4(const float *x, float *y, int n, int h, int w, hipStream_t s);
// exact GELU in place over n4 16-byte quads
hipError_t launch_gelu(float *x, int64_t n4, hipStream_t s);

// TDN-ResNet50 (tsm_tdn.hip), fp32 NHWC.  The mSE launches take conv1's width c in {128, 256, 512} (r = c / 16 channels in
// between); anything else hipErrorInvalidValue, nothing launched.  Weight layouts: tsm_host::tdn_pack_mse.
// front: x [n, 15, h, w] (h, w multiples of 32, >= 64; n <= 65535) -> in4 [n, h, w, 4] (the centre frame, packed) and the patch
// rows of conv1_5 [n * h / 4 * w / 4][tsm_host::kTdnPatchK]
hipError_t launch_tdn_front(const float *x, float *in4, float *patches, int n_frames, int h, int w, hipStream_t s);
hipError_t launch_tdn_front_pool(const tsm_host::TdnPoolSource &src, float *in4, float *patches, int n_segments, int h, int w, hipStream_t s);
// x [n, h, w, c] <- alpha x + beta nearest-upsampled d [n, hd, wd, c], in place
hipError_t launch_tdn_fuse(float *x, const float *d, int n, int h, int w, int hd, int wd, int c, float alpha, float beta, hipStream_t s);
// x [n, h, w, c] = alpha ring_a[slot] + beta nearest-upsampled ring_d[slot], slot = tsm_host::tdn_ring_slot(table[segment], n_slots)
// (device int32 [n]); a slot outside the ring stands for zeros
hipError_t launch_tdn_fuse_ring(const float *ring_a, const float *ring_d, const int32_t *table, int n_slots, float *x, int n, int h, int w,
                                int hd, int wd, int c, float alpha, float beta, hipStream_t s);
// b [m, r] = BN(W1 x), x [m, c]
hipError_t launch_mse_squeeze(const float *x, const float *wq, const float *bq, float *b, int64_t m, int c, hipStream_t s);
// d+ / d- [n, h, w, r] and their 2x2 average pools pf / pb [n, h / 2, w / 2, r] from b; n = clips * T
hipError_t launch_mse_diff(const float *b, const float *dw, float *df, float *db, float *pf, float *pb, int n_frames, int T, int h, int w,
                           int c, hipStream_t s);
// s2 = BN(K2 * pooled d) on the pooled map, both directions
hipError_t launch_mse_s2(const float *pf, const float *pb, const float *k2, const float *b2, float *sf, float *sb, int n_frames, int hp, int wp,
                         int c, hipStream_t s);
// m = d / 3 + up(s2) / 3 + BN(K4 * d) / 3, both directions
hipError_t launch_mse_mix(const float *df, const float *db, const float *s2f, const float *s2b, const float *k4, const float *b4, float *mf,
                          float *mb, int n_frames, int h, int w, int c, hipStream_t s);
// o = temporal conv of g = x + x y, y from e = BN(W3 m); x, o [n_clips * T, hw, c]; n_clips <= 65535
hipError_t launch_mse_excite_shift(const float *x, const float *mf, const float *mb, const float *w3, const float *b3, const float *wt, float *o,
                                   int n_clips, int T, int hw, int c, hipStream_t s);

// K9: per clip, (softmax,) first arg-max, class id if its score >= threshold else -1; top (nullable) = that score.
hipError_t launch_scores_to_states(const float *logits, int n, int c, int softmax, float threshold, int *states, float *top,
                                   hipStream_t s);

// Launch trace of the calling thread (tsm_trace_launches / tsm_launch_trace in include/tsm_hip.h; tsm_ops.hip).
// reverse: -1 for a kernel without a tile walk; 0 / 1 the direction of one that has one (1 appends " [reverse]")
// mark: a bracket about the launch's grid, in front of the direction's (" [balanced 1792/1280]": live-balanced XCD runs,
// workgroups of the whole part / whole tiles), so that a line still ends as it did
void note_launch(const char *kernel, const char *where, int reverse = -1, const char *mark = nullptr);
void trace_launches(bool on);
const char *launch_trace();   // newline-separated, valid until the thread's next trace call

}  // namespace tsm
