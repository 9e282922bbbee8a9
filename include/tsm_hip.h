/*
 * tsm_hip.h -- C ABI of libtsm_hip.so: TSM-ResNet50 (and ResNet-18 / 34) clip inference on MI355X (gfx950).
 *
 * The reference (iucario/WorkoutDetector) has no FFI of its own: the hot path sits behind a
 * Python duck type.  Each entry point below names the reference interface it replaces:
 *
 *   tsm_create / tsm_set_tensor / tsm_finalize
 *       create_model(num_class, num_segments, base_model='resnet50', checkpoint, ...)
 *       workoutdetector/models/tsm.py:422-476  (state-dict keys of TSM, tsm.py:250-262)
 *       and onnxruntime.InferenceSession(ckpt) workoutdetector/utils/inference_count.py:620
 *   tsm_forward
 *       model.run(None, {input_name: float32[1,8,3,224,224]}) -> [float32[1,num_class]]
 *       workoutdetector/utils/inference_count.py:273-275, scripts/eval_classification.py:43-44
 *       == TSM.forward(x[B*T,3,H,W]) -> [B,num_class]   workoutdetector/models/tsm.py:409-419
 *       ([B,T,num_class] with consensus_type='identity', tsm_set_consensus)
 *   tsm_tune               (no counterpart: onnxruntime optimises its graph inside InferenceSession(), :620; this is the
 *                          engine's per-batch-size kernel selection, made callable ahead of the first request)
 *   tsm_forward_tap        (parity tests) activation after a named stage of TSM.forward
 *   tsm_temporal_shift     TemporalShift.shift          workoutdetector/models/tsm.py:35-50
 *   tsm_conv_bn_act        one conv + BatchNorm(eval) [+ residual] [+ ReLU] of the torchvision
 *                          Bottleneck kept by TSM        workoutdetector/models/tsm.py:250-251,264-281
 *   tsm_conv_op            the same with the engine's other conv forms (shifted identity, conv3 + downsample, tile code)
 *   tsm_maxpool3x3s2       base_model.maxpool
 *   tsm_head               avgpool -> fc -> view(-1,T,cls) -> mean(1)   tsm.py:411-419,165-174
 *   tsm_set_consensus      create_model(consensus_type='avg' | 'identity')   workoutdetector/models/tsm.py:438,165-174
 *   tsm_head_segments      avgpool -> fc -> view(-1,T,cls), SegmentConsensus('identity'): no mean   tsm.py:411-419,165-174
 *   tsm_gather_clips       the loop's clip windows: video[i:i + 16:2] for i in range(0, len(video), 8), zero-padded tail
 *   tsm_preprocess_clips   build_test_transform(person_crop=True) from the detector's box on: PersonCrop -> Resize((224, 224))
 *                          -> Normalize, fused with the clip windows   datasets/build.py:123-129, datasets/transform.py:247-259
 *   tsm_preprocess_indexed build_test_transform(person_crop=False) over FrameDataset's sampled frames: one launch from staged raw
 *                          frames through a device index table (sample_frames(total, 8, start, random=False) per labelled
 *                          segment)   datasets/common.py:99-117, datasets/transform.py:16-65, datasets/build.py:131-136
 *   tsm_preprocess_windows either test transform over the windows of one step of a stream server: frame sizes differ per
 *                          window, optional person box per window   utils/inference_count.py:285-339, app/inference.py:87-111
 *   tsm_scores_to_states   per clip: to_softmax, first arg-max, score >= 0.5 ? class : -1
 *                          workoutdetector/utils/eval.py:153-164, utils/visualize.py:140-150
 *   tsm_preprocess_image   data_transform of the image model: ToPILImage -> Resize(256) -> CenterCrop(224) -> ToTensor -> Normalize
 *                          (Pillow's antialiased resample, to the bit)   workoutdetector/utils/inference_count.py:27-34,168-189
 *   tsm_frame_votes        count_by_image_model's vote: arg-max per frame, deque of 7, sum(que) >= 4
 *                          workoutdetector/utils/inference_count.py:221-231
 *   tsm_top1_tally         the comparison of the accuracy loop: arg-max == label, counted per class (the loop's intent: the
 *                          snapshot compares a logits row and never counts the totals)   scripts/eval_classification.py:42-49
 *   tsm_forward_features   cnn_feature / video_feature: timm.create_model(name, num_classes=0)(frames) -> the pooled vector of
 *                          every frame   workoutdetector/utils/common.py:79-116
 *   tsm_pool_features      the global average pool such a model ends in, and sklearn's normalize() of its rows
 *   tsm_cosine_distances   plot_sim: pairwise_distances(feats, metric='cosine'), the temporal self-similarity matrix
 *                          workoutdetector/utils/common.py:118-143
 *
 * Conventions
 *   - Plain pointers and sizes only; no torch / HIP types in signatures.  hip streams travel as
 *     void*.  NULL means: the device's default (null) stream for TSM_MEM_DEVICE calls and per-op
 *     entry points (so work is ordered after whatever produced the buffers there -- torch's default
 *     stream is the null stream), the engine's private stream for TSM_MEM_HOST calls.
 *   - Every function returns 0 on success or a negative tsm_status; the message for the last
 *     failure on an engine is tsm_last_error(engine) (engine == NULL: the calling THREAD's last failure of
 *     tsm_create or of an engine-less per-op entry point; no process-global state).
 *   - An engine owns its weights and workspace on ONE device; it is NOT re-entrant: one
 *     in-flight call per engine.  Independent engines (other devices / processes) coexist.
 *   - Caller owns all input / output buffers.  With TSM_MEM_HOST the call copies and
 *     synchronises before returning; with TSM_MEM_DEVICE the call only enqueues on `stream` -- with ONE
 *     exception: the FIRST tsm_forward of a new power-of-two bucket of n_clips tunes its kernels first (unless
 *     TSM_AUTOTUNE=0, or TSM_TUNE_CACHE names a file that already holds this bucket): it times every candidate on the
 *     real launches, which synchronises with `stream` about a hundred times and takes a few hundred ms, so that call is
 *     neither asynchronous nor legal inside a stream capture.  Call tsm_tune per bucket at start-up (TsmEngine.warmup
 *     in the Python host) before capturing a graph or relying on enqueue-only behaviour; every later call of that
 *     bucket allocates nothing, synchronises nothing and is capture-safe.
 *   - Activations inside the engine are NHWC fp32.
 */
#ifndef TSM_HIP_H_
#define TSM_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSM_ABI_VERSION 7 /* 7: tsm_build_id, tsm_set_backbone, tsm_set_bottleneck_width, tsm_set_consensus, tsm_head_segments, tsm_preprocess_clips, tsm_preprocess_image, tsm_frame_votes, tsm_preprocess_indexed, tsm_top1_tally, tsm_forward_features, tsm_pool_features, tsm_cosine_distances (all nine added later within 7: no existing entry point changed), tsm_set_shift_place, tsm_conv_op, tsm_trace_launches / tsm_launch_trace; 6: tsm_tune, per-user default tune cache; 5: tsm_gather_clips; 4: tsm_scores_to_states; tile codes lost the tail field; TSM_* variables read in tsm_create only */

typedef enum tsm_status {
  TSM_OK = 0,
  TSM_ERR_INVALID_ARG = -1,
  TSM_ERR_HIP = -2,
  TSM_ERR_NOT_FINALIZED = -3,
  TSM_ERR_MISSING_TENSOR = -4,
  TSM_ERR_SHAPE = -5,
  TSM_ERR_CAPACITY = -6,
  TSM_ERR_UNSUPPORTED = -7,
  TSM_ERR_GUARD = -8 /* hostile-memory check (tsm_conv_op always; an engine under TSM_POISON=1): a launch stored into the poisoned
                        band before or after a device buffer; the message names buffer, side and element offset.  Additive:
                        no existing entry point changed, TSM_ABI_VERSION stays 7 */
} tsm_status;

typedef enum tsm_memkind { TSM_MEM_HOST = 0, TSM_MEM_DEVICE = 1 } tsm_memkind;

/* Layout of the clip tensor handed to tsm_forward (T = num_segments). */
typedef enum tsm_layout {
  TSM_LAYOUT_NTCHW = 0, /* float32 [B,T,3,H,W]  -- the reference's ONNX input; the stem kernel reads it as it is
                           (rounds / splits while it stages its patch: no packed copy, no extra launch)           */
  TSM_LAYOUT_NTHWC = 1, /* float32 [B,T,H,W,3]  -- decoder-native, skips the host permute */
  TSM_LAYOUT_NTHWC4 = 2, /* float32 [B,T,H,W,4]  -- what tsm_preprocess writes for a TSM_DTYPE_F32 engine
                            (4th channel 0: the stem never reads it); device memory only, consumed in place without a repack */
  TSM_LAYOUT_NTHWC8S = 3, /* split-bf16 [B,T,H,ceil(W/2),8]: one 32-byte group [hi x8 | lo x8] per PIXEL PAIR,
                             elements (pixel 2j: c0 c1 c2 0, pixel 2j+1: c0 c1 c2 0), an odd width ends in a
                             zero pixel -- what tsm_preprocess writes for a TSM_DTYPE_BF16X3 engine (the 7x7
                             stride-2 stem then reads 4 aligned pairs per kernel row); device memory only */
  TSM_LAYOUT_NTHWC8B = 4, /* bf16 [B,T,H,ceil(W/2),8]: the same pixel pairs, 16 bytes per pair -- for a
                             TSM_DTYPE_BF16 engine */
  TSM_LAYOUT_TDN_POOL = 16, /* a TDN engine only: `clips` points to a tsm_tdn_pool in HOST memory (below, beside tsm_set_tdn), which
                               names a pool of transformed frames in device memory; memkind must be TSM_MEM_DEVICE.  Not an
                               out_layout of the tsm_preprocess* entry points */
  TSM_LAYOUT_TDN_SEGMENTS = 17, /* a TDN engine only, the SEGMENT phase of the two-phase forward (beside tsm_set_tdn): `clips` points
                                   to a tsm_tdn_segments in HOST memory; n_clips counts segments; memkind must be TSM_MEM_DEVICE */
  TSM_LAYOUT_TDN_RING = 18 /* a TDN engine only, the TRUNK phase: `clips` points to a tsm_tdn_ring in HOST memory naming a ring of
                              per-segment features and a table of slot numbers in device memory; memkind must be TSM_MEM_DEVICE */
} tsm_layout;

/* The input of a TDN forward as a pool of frames (TSM_LAYOUT_TDN_POOL; the contract stands beside tsm_set_tdn). */
typedef struct tsm_tdn_pool {
  uint32_t struct_size;        /* sizeof(tsm_tdn_pool) */
  int32_t mode;                /* 0 table, 1 window */
  const float *frames;         /* device, [n_frames, 3, H, W], H x W the engine's, 8-byte aligned */
  int64_t n_frames;
  const int32_t *index;        /* mode 0: device, [n_clips, T, 5] */
  int64_t first_source_frame, total_frames, first_clip; /* mode 1 */
  int32_t clip_step, clip_stride;                       /* mode 1 */
  int64_t pad_frame;           /* mode 1: pool frame standing for "no frame"; < 0 or >= n_frames: zero planes */
} tsm_tdn_pool;

/* The segment phase of a TDN forward (TSM_LAYOUT_TDN_SEGMENTS): where the frames are -- tsm_tdn_pool's fields, one SEGMENT where
 * that struct has a clip -- and where the two per-segment feature maps go. */
typedef struct tsm_tdn_segments {
  uint32_t struct_size;        /* sizeof(tsm_tdn_segments) */
  int32_t mode;                /* 0 table, 1 window */
  const float *frames;         /* device, [n_frames, 3, H, W], 8-byte aligned */
  int64_t n_frames;
  const int32_t *index;        /* mode 0: device, [n, 5] */
  int64_t first_source_frame, total_frames, first_clip; /* mode 1: segment i has centre clip_stride * (first_clip + i) */
  int32_t clip_step, clip_stride;                       /* mode 1 (clip_step is not read: a segment is its own clip) */
  int64_t pad_frame;           /* mode 1, as tsm_tdn_pool's */
  float *out_a;                /* device, [n, H / 4, W / 4, 256]: layer1's output before the blend; 16-byte aligned */
  float *out_d;                /* device, [n, H / 8, W / 8, 256]: resnext_layer1's output; 16-byte aligned */
} tsm_tdn_segments;

/* The trunk phase of a TDN forward (TSM_LAYOUT_TDN_RING): segment k of clip c is slot table[c * T + k] of the ring. */
typedef struct tsm_tdn_ring {
  uint32_t struct_size;        /* sizeof(tsm_tdn_ring) */
  int32_t n_slots;             /* > 0 */
  const float *ring_a;         /* device, [n_slots, H / 4, W / 4, 256], 16-byte aligned */
  const float *ring_d;         /* device, [n_slots, H / 8, W / 8, 256], 16-byte aligned */
  const int32_t *table;        /* device, int32 [n_clips, T] of slot numbers; an entry outside [0, n_slots) stands for zeros */
} tsm_tdn_ring;

/* The staged frames of a frame transform (tsm_preprocess, _clips, _indexed, _windows).
 *   TSM_PIXEL_U8 / TSM_PIXEL_F32   [h, w, 3] RGB, values 0..255.
 *   TSM_PIXEL_NV12_*               what a hardware decoder leaves: h * w luma bytes, then h / 2 rows of w bytes of interleaved
 *     (U, V) pairs -- dense (no pitch; the chroma plane follows the luma plane directly), h and w even, 3 h w / 2 bytes per
 *     frame, frames of a buffer at that distance.  Converted inside the transform's taps, never written as RGB: luma pixel
 *     (y, x) takes the pair at chroma row y >> 1, bytes 2 (x >> 1) and 2 (x >> 1) + 1 (nearest-neighbour chroma, as
 *     cv2.COLOR_YUV2RGB_NV12), and with C = Y - y_off, D = U - 128, E = V - 128, in int32 with an arithmetic shift:
 *       R = clamp((cy C + crv E + 8192) >> 14, 0, 255)
 *       G = clamp((cy C + cgu D + cgv E + 8192) >> 14, 0, 255)
 *       B = clamp((cy C + cbu D + 8192) >> 14, 0, 255)
 *                       y_off     cy    crv    cgu     cgv    cbu
 *       BT601 (limited)    16  19077  26149  -6419  -13320  33050
 *       BT709 (limited)    16  19077  29372  -3494   -8731  34610
 *       BT601_FULL          0  16384  22970  -5638  -11700  29032
 *       BT709_FULL          0  16384  25802  -3069   -7670  30402
 *     Everything behind the conversion (bilinear taps, zero fill, normalisation) is the RGB transform's, bit for bit that of
 *     the converted frame.
 *   TSM_PIXEL_I420_* .. TSM_PIXEL_UYVY_*   code 32 + 4 f + c: f the format (I420 0, YV12 1, P010 2, YUYV 3, UYVY 4), c the
 *     coefficient row in the order above.  What other sources leave; all dense, converted in the taps by the same formula,
 *     bit for bit the RGB transform of the converted frame.
 *       I420 (a software decoder's yuv420p): h * w Y bytes, then h/2 * w/2 U bytes, then h/2 * w/2 V bytes; 3 h w / 2 bytes,
 *         h and w even; pixel (y, x) takes U and V at (y >> 1, x >> 1) of their planes.  YV12: the V plane before the U plane.
 *       P010 (a 10-bit decode): NV12's arrangement with 16-bit little-endian samples, the 10 significant bits in the most
 *         significant bits; 3 h w bytes, h and w even, `frames` 4-byte aligned.  A sample enters the formula as its HIGH byte
 *         (word >> 8) and the low byte is ignored whatever it holds: everything downstream is the 8-bit RGB pipeline, so a
 *         P010 frame equals, bit for bit, the NV12 frame made of its high bytes.
 *       YUYV (a capture device's packed 4:2:2): h rows of w / 2 groups of the bytes (Y0, U, Y1, V); 2 h w bytes, w even,
 *         any h >= 1, `frames` 4-byte aligned; the two pixels of a group share its U and V, rows share nothing.  UYVY: the
 *         bytes of a group are (U, Y0, V, Y1).
 *     Codes 2..15, 20..31 and 52 on are invalid. */
typedef enum tsm_pixel {
  TSM_PIXEL_U8 = 0,
  TSM_PIXEL_F32 = 1,
  TSM_PIXEL_NV12_BT601 = 16,
  TSM_PIXEL_NV12_BT709 = 17,
  TSM_PIXEL_NV12_BT601_FULL = 18,
  TSM_PIXEL_NV12_BT709_FULL = 19,
  TSM_PIXEL_I420_BT601 = 32,
  TSM_PIXEL_I420_BT709 = 33,
  TSM_PIXEL_I420_BT601_FULL = 34,
  TSM_PIXEL_I420_BT709_FULL = 35,
  TSM_PIXEL_YV12_BT601 = 36,
  TSM_PIXEL_YV12_BT709 = 37,
  TSM_PIXEL_YV12_BT601_FULL = 38,
  TSM_PIXEL_YV12_BT709_FULL = 39,
  TSM_PIXEL_P010_BT601 = 40,
  TSM_PIXEL_P010_BT709 = 41,
  TSM_PIXEL_P010_BT601_FULL = 42,
  TSM_PIXEL_P010_BT709_FULL = 43,
  TSM_PIXEL_YUYV_BT601 = 44,
  TSM_PIXEL_YUYV_BT709 = 45,
  TSM_PIXEL_YUYV_BT601_FULL = 46,
  TSM_PIXEL_YUYV_BT709_FULL = 47,
  TSM_PIXEL_UYVY_BT601 = 48,
  TSM_PIXEL_UYVY_BT709 = 49,
  TSM_PIXEL_UYVY_BT601_FULL = 50,
  TSM_PIXEL_UYVY_BT709_FULL = 51
} tsm_pixel;

/* Arithmetic of the conv stack.
 *   TSM_DTYPE_F32     fp32 storage, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): bit-for-bit an fp32 fma chain.
 *   TSM_DTYPE_BF16X3  "split-bf16": every activation/weight is kept as hi = bf16(x), lo = bf16(x - hi)
 *                     (4 bytes per element, like fp32) and a*b is computed as ah*bh + ah*bl + al*bh on
 *                     the bf16 MFMA with fp32 accumulation: ~2^-17 relative error per product (fp32-class
 *                     results, within the path's rtol 1e-3 with >10x margin) at several times the speed.
 *   TSM_DTYPE_BF16    bf16 weights and activations, one bf16 MFMA per product, fp32 accumulate
 *                     (BASELINE.json config 5, the roofline stress config).  NOT within rtol 1e-3 of the
 *                     fp32 reference: ~1e-2 relative on logits; tests state the tolerance. */
typedef enum tsm_dtype { TSM_DTYPE_F32 = 0, TSM_DTYPE_BF16X3 = 1, TSM_DTYPE_BF16 = 2 } tsm_dtype;

typedef struct tsm_config {
  int32_t struct_size;  /* = sizeof(tsm_config), ABI guard                           */
  int32_t num_class;    /* 12 for the RepCount 6-action x 2-state model              */
  int32_t num_segments; /* T, 8 (16 for the stress config)                           */
  int32_t height;       /* 224                                                       */
  int32_t width;        /* 224                                                       */
  int32_t shift_div;    /* 8: fold = C / shift_div.  TSM_DTYPE_F32: 1, 2, 4, 8 or 16; the
                           bf16 formats: 1, 2, 4 or 8 (whole 8-channel groups); anything
                           else TSM_ERR_UNSUPPORTED.  Channels [0, fold) of a shifted
                           tensor read frame t + 1, [fold, 2 fold) frame t - 1, the rest
                           frame t.  2: no channel reads its own frame.  1: fold = C, every
                           channel reads t + 1 and the t - 1 group is empty (the
                           reference's slicing); blockres placement only, see
                           tsm_set_shift_place                                          */
  int32_t is_shift;     /* 1: temporal shift in front of every Bottleneck.conv1      */
  int32_t max_clips;    /* workspace capacity in clips per tsm_forward call          */
  int32_t device_id;    /* HIP device ordinal                                        */
  int32_t dtype;        /* TSM_DTYPE_F32 | TSM_DTYPE_BF16X3 | TSM_DTYPE_BF16         */
} tsm_config;

typedef struct tsm_engine tsm_engine;

int tsm_abi_version(void);

/* The identity of the SOURCE this binary was built from: the first 16 hex digits of the sha256 over csrc/ (file names,
 * contents, per-file compiler options) and the extra compiler definitions of the build -- what
 * workoutdetector_amd/build.py::build_id() computes from the tree.  The library is git-ignored and travels prebuilt, so
 * the Python host refuses one whose id is not the tree's (workoutdetector_amd/_lib.py) and bench.py prints it; it also
 * keys the tune cache.  A hand build without -DTSM_BUILD_ID reports its compile time stamp.
 * (No counterpart in the reference: a Python package cannot be stale against itself.) */
const char *tsm_build_id(void);

/* Launch trace of the CALLING THREAD (parity tests: "did the kernel under test really run?").  tsm_trace_launches(1)
 * clears the thread's trace and starts recording one line per kernel launch this library makes from that thread -- the
 * kernel's name as rocprofv3 would print it up to template-argument spelling, e.g. "bneck_ws_kernel<256, true, true>" or
 * "conv_igemm<BM, BN, WGM, WGN, KS, SHIFT, RES, kPrecBf16> [BM = 64, BN = 64, ...]"; tsm_trace_launches(0) stops.
 * tsm_launch_trace copies the newline-separated trace (NUL-terminated) into buf when cap suffices and always returns the
 * bytes needed.  A kernel that walks its output tiles / frames in a direction (conv_igemm, conv_bf16_256[p], the weight-
 * stationary convs, bneck_ws, front_s2, conv31, conv23) ends its line with " [reverse]" when it walks from the far end:
 * appended after everything else, so the line still ends in ']' and every prefix of it is unchanged.  A forward walk, and
 * every launch without a walk, leaves the line as above.
 * Off by default; per thread, like the engine-less error message: no process-global state.
 * (No counterpart in the reference: onnxruntime's session.run is opaque, utils/inference_count.py:273-275.) */
int tsm_trace_launches(int32_t on);
int64_t tsm_launch_trace(char *buf, int64_t cap);

/* Engine lifetime ------------------------------------------------------------------------- */
int tsm_create(const tsm_config *cfg, tsm_engine **out);
void tsm_destroy(tsm_engine *e);
const char *tsm_last_error(const tsm_engine *e);

/* Backbone of the engine: torchvision's resnet18 / resnet34 (BasicBlock: two 3x3 convs, the temporal shift fused into
 * the first, fc [num_class, 512]) or resnet50 (Bottleneck, fc [num_class, 2048]) -- create_model(base_model=...),
 * workoutdetector/models/tsm.py:264-281.  Legal between tsm_create and the first tsm_set_tensor; a later call returns
 * TSM_ERR_INVALID_ARG, a depth other than 18, 34 or 50 TSM_ERR_UNSUPPORTED.  An engine that never calls it is R50.
 * State-dict keys of a BasicBlock: "base_model.layerL.B.conv1.net.weight" (or ".conv1.weight"), ".bn1.*",
 * ".conv2.weight", ".bn2.*", ".downsample.0.weight", ".downsample.1.*". */
int tsm_set_backbone(tsm_engine *e, int32_t depth);

/* Bottleneck width of the engine: torchvision's width_per_group.  64 (default: every Bottleneck's mid width is its stage's
 * planes, 64 / 128 / 256 / 512) or 128 (wide_resnet50_2: mid widths 128 / 256 / 512 / 1024, block outputs still 256 / 512 /
 * 1024 / 2048, the same state-dict keys as resnet50).  Same contract as tsm_set_backbone: legal between tsm_create and the
 * first tsm_set_tensor, later TSM_ERR_INVALID_ARG; any other value TSM_ERR_UNSUPPORTED, and so is 128 together with a
 * BasicBlock depth (18 / 34), whichever of the two calls comes second -- torchvision refuses base_width != 64 there. */
int tsm_set_bottleneck_width(tsm_engine *e, int32_t width_per_group);

/* Placement of the temporal shift -- create_model(shift_place=...), workoutdetector/models/tsm.py:104-124:
 * 0 = 'blockres' (default: the shift wraps conv1 of every block, the identity sees the unshifted input), 1 = 'block' (it
 * wraps every block of layer1-4 whole: conv1, the identity and the downsample all read the shifted input).  is_shift = 0
 * ignores it, as the reference does.  Same contract as tsm_set_backbone: legal between tsm_create and the first
 * tsm_set_tensor, later TSM_ERR_INVALID_ARG; any other value TSM_ERR_UNSUPPORTED.  place = 1 on an engine created with
 * is_shift = 1 and shift_div = 1 is TSM_ERR_UNSUPPORTED with a message: the shifted identity and downsample launches need both
 * channel groups inside the tensor (2 * fold <= channels), so such an engine could not run a forward.  State-dict keys of a block engine:
 * "base_model.layerL.B.net.<name>" (or the un-wrapped "base_model.layerL.B.<name>"); a blockres "conv1.net" key is unknown. */
int tsm_set_shift_place(tsm_engine *e, int32_t place);

/* Segment consensus of the head -- create_model(consensus_type=...), workoutdetector/models/tsm.py:438,165-174:
 * 0 = 'avg' (default: the mean of the segments' fc outputs, logits [n_clips, num_class]), 1 = 'identity' (the fc output of
 * every segment, logits [n_clips, num_segments, num_class]; one launch, head_seg_kernel).  Same contract as
 * tsm_set_shift_place: legal between tsm_create and the first tsm_set_tensor, later TSM_ERR_INVALID_ARG; any other value
 * TSM_ERR_UNSUPPORTED.  It changes neither a weight nor a conv launch, and the tune cache does not carry it: a cache line
 * written by an avg engine serves an identity engine of the same geometry. */
int tsm_set_consensus(tsm_engine *e, int32_t consensus);

/* Non-local blocks -- create_model(non_local=True), the TSM code base's make_non_local: on = 1 wraps blocks 0 and 2 of layer2
 * and blocks 0, 2 and 4 of layer3 in an embedded-Gaussian non-local block.  With x [B*T, C, H, W] the wrapped block's (post-ReLU)
 * output and d = C / 2: theta = conv1x1x1(x), phi = g = conv1x1x1(x) followed by MaxPool3d((1, 2, 2)) (floor mode), the
 * T*H*W x T*(H/2)*(W/2) scores f = theta^T phi without a scale factor, y = softmax_j(f) g, z = BN(conv1x1x1(y)) + x without a
 * ReLU; z is the wrapped block's output.  The scores are never materialised (nonlocal_attn_kernel: online softmax).
 * State-dict keys of a wrapped block: its own tensors under "base_model.layerL.B.block.<name>" (the spelling without ".block"
 * is accepted too), and "base_model.layerL.B.nl.{theta, phi.0, g.0}.{weight [d, C, 1, 1, 1], bias}", "...nl.W.0.{weight
 * [C, d, 1, 1, 1], bias}", "...nl.W.1.{weight, bias, running_mean, running_var}".  Taps: "layerL.B" is z, "layerL.B.block" the
 * block's own output, "layerL.B.nl.y" is y.
 * Same contract as tsm_set_shift_place: legal between tsm_create and the first tsm_set_tensor, later TSM_ERR_INVALID_ARG.
 * TSM_ERR_UNSUPPORTED, whichever call comes second: a dtype other than TSM_DTYPE_F32, a BasicBlock backbone (depth 18 / 34). */
int tsm_set_non_local(tsm_engine *e, int32_t on);

/* Temporal pool -- create_model(temporal_pool=True), the TSM code base's make_temporal_pool: on = 1 wraps layer2 in
 * TemporalPool.  With x [B*T, C, H, W] layer1's output viewed [B, T, C, H, W], the pool is max_pool3d with kernel (3, 1, 1),
 * stride (2, 1, 1), padding (1, 0, 0): output frame t' in [0, T/2) of a clip is the elementwise max over its source frames
 * {2t'-1, 2t', 2t'+1} cut to [0, T); a frame of another clip is never read.  One launch of its own (temporal_maxpool_kernel),
 * bit-exact in the storage format.  Layers 2-4 then run on B*T/2 frames and shift over T/2 segments (layer1 keeps T, in both
 * placements; with T = 2 the later stages have one segment and the shifted channels are zero); the head's consensus runs
 * over T/2 frames: tsm_forward writes [n_clips, num_class] (avg) or [n_clips, T/2, num_class] (identity),
 * tsm_forward_features [n_clips * T/2, feat_dim], and every tap from layer2 on has n_clips * T/2 frames.  The tap
 * "layer2.tpool" is the pooled tensor; the launch has a timing slot of that name behind layer1's last block.
 * No new tensors.  State-dict keys of layer2 under the wrapper: "base_model.layer2.net.<b>.<rest>" (the wrapper holds the
 * stage as `net`), accepted beside the plain "base_model.layer2.<b>.<rest>".
 * Same contract as tsm_set_shift_place: legal between tsm_create and the first tsm_set_tensor, later TSM_ERR_INVALID_ARG; a
 * value other than 0 or 1 TSM_ERR_UNSUPPORTED.  on = 1 is TSM_ERR_UNSUPPORTED on a TSM_DTYPE_BF16 engine (its cross-block
 * and whole-block kernels tile over all T frames of a clip), with is_shift = 0, with an odd num_segments, and together with
 * tsm_set_non_local(e, 1), whichever of the two calls comes second (the non-local wrapper assumes one segment count). */
int tsm_set_temporal_pool(tsm_engine *e, int32_t on);

/* ConvNeXt image model -- create_image_model(base_model='convnext_base'): the engine builds a ConvNeXt topology (timm 0.5.4
 * convnext_base: widths 128 / 256 / 512 / 1024, depths[s] blocks in stage s, (3, 3, 27, 3) for the model itself) in place
 * of the ResNet one.  Input [n, 3, H, W], one frame per clip.  Stem: Conv2d(3, 128, k 4, s 4) + LayerNorm; stages 1 .. 3 start
 * with LayerNorm + Conv2d(C / 2, C, k 2, s 2) (floor mode: a last odd row / column is dropped); a block is
 * x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x))))) with an exact (erf) GELU and no activation behind the add; the head is the mean
 * over the pixels, LayerNorm, fc.  Every LayerNorm is over the channels of one pixel, biased variance, eps 1e-6, affine.
 * Launches: the depthwise 7x7 and its LayerNorm are one kernel (dwconv7_ln_kernel); the stem, the downsamples, fc1 and fc2 run
 * on conv_igemm as 1x1 convs (the layer scale gamma folded into fc2, the residual in its epilogue); GELU is an in-place pass.
 * State-dict keys, timm's: "stem.0.{weight [128, 3, 4, 4], bias}", "stem.1.{weight, bias}", "stages.S.downsample.0.{weight,
 * bias}" (LayerNorm) and "stages.S.downsample.1.{weight [C, C / 2, 2, 2], bias}" for S = 1 .. 3, "stages.S.blocks.B.conv_dw.{weight
 * [C, 1, 7, 7], bias}", "....norm.{weight, bias}", "....mlp.fc1.{weight [4 C, C], bias}", "....mlp.fc2.{weight [C, 4 C], bias}",
 * "....gamma [C]", "head.norm.{weight, bias}", "head.fc.{weight [num_class, 1024], bias}".
 * tsm_forward writes [n_clips, num_class]; tsm_forward_features [n_clips, 1024], the head LayerNorm's output (normalize: each
 * row over its Euclidean norm).  Taps: "stem", "stages.S.downsample", "stages.S.blocks.B" (the block's output), "....dwln" (the
 * normalised depthwise output), "....fc1" (behind the GELU), "head.pool", "head.norm".
 * Legal between tsm_create and the first tsm_set_tensor, later TSM_ERR_INVALID_ARG (as is depths == NULL).
 * TSM_ERR_UNSUPPORTED: num_segments != 1, is_shift != 0, a dtype other than TSM_DTYPE_F32, a depth outside 1 .. 64, and after
 * tsm_set_backbone, tsm_set_bottleneck_width, tsm_set_shift_place, tsm_set_non_local(e, 1) or tsm_set_temporal_pool(e, 1);
 * those five are TSM_ERR_UNSUPPORTED in turn on an engine that is already a ConvNeXt one. */
int tsm_set_convnext(tsm_engine *e, const int32_t depths[4]);

/* TDN-ResNet50 (Temporal Difference Network) -- create_model of workoutdetector/models/tdn.py: TSN(backbone_fn=tdn_net).  The
 * engine builds the TDN topology in place of the TSM one.  Eval mode, fp32.  This comment is the network's definition.
 *
 * Input [n_clips, T, 5, 3, H, W] = [n_clips, T, 15, H, W] = [n_clips * T * 5, 3, H, W] (one memory layout): f0 .. f4 are the five
 * frames of a segment, N = n_clips * T.
 * Short-term path:  D = concat(f1 - f0, f2 - f1, f3 - f2, f4 - f3) (12 channels); P = avgpool2x2(D), stride 2;
 *   x_c5 = ReLU(BN(conv7x7 s2 p3 (P))), 12 -> 64, no conv bias ("base_model.conv1_5.0.weight" [64, 12, 7, 7], BN "conv1_5.1.*");
 *   xd0 = maxpool3x3 s2 p1 (x_c5); xd1 = resnext_layer1(xd0): depths[0] plain Bottlenecks 64 -> 256 with their own weights.
 * Trunk:  s = maxpool(ReLU(BN(conv1(f2)))) -- the stem sees the centre frame only; x = alpha s + beta up(xd0); x = layer1_bak(x)
 *   (plain Bottlenecks); x = alpha x + beta up(xd1); layer2_bak .. layer4_bak are BottleneckShift blocks; global average pool,
 *   new_fc, consensus over T.  up is torch's 'nearest' to the target size: src = min(int(floorf(dst * ((float)in / out))), in - 1).
 *   alpha, beta are arguments (tdn_net's rule: 0.5, 0.5 when T == 8, else 0.75, 0.25).
 * Every conv of both ResNets (conv1, the block convs, the downsamples) has a bias and a BatchNorm behind it (eps 1e-5); a
 * Bottleneck is torchvision's with the stride on conv2.
 * BottleneckShift: conv1 + BN + ReLU, mse, shift, conv2 (3x3 at the block's stride) + BN + ReLU, conv3 + BN (+ downsample), add,
 * ReLU.  With x = conv1's output [N, H, W, C] and r = C / 16:
 *   b = BN_a(W1 x), 1x1 C -> r, no bias ("mse.conv1", "mse.bn1");  c = DW3x3(b), depthwise, pad 1, no bias, no BN ("mse.conv2" [r, 1, 3, 3]);
 *   d+[t] = c[t + 1] - b[t] for t < T - 1 and 0 at t = T - 1;  d-[t] = c[t - 1] - b[t] for t > 0 and 0 at t = 0; frames of another
 *   clip are never read.  For each direction d:
 *     s2 = BN_2(K2 * avgpool2x2(d)), the pool in floor mode (7 -> 3), K2 a full 3x3 r -> r, pad 1, no bias
 *          ("mse.conv3_smallscale2", "mse.bn3_smallscale2");  s4 = BN_4(K4 * d) at full size ("mse.conv3_smallscale4", "mse.bn3_smallscale4");
 *     m = d / 3 + up(s2) / 3 + s4 / 3 -- the BatchNorm biases make m non-zero on the zero frame: it is not skipped;
 *   e = BN_3(W3 m), 1x1 r -> C, no bias ("mse.conv3", "mse.bn3"; the same weights for both directions);
 *   y = (sigmoid(e+) - 1/2) / 2 + (sigmoid(e-) - 1/2) / 2;  g = x + x y;
 *   o[t, c] = w[c, 0] g[t - 1, c] + w[c, 1] g[t, c] + w[c, 2] g[t + 1, c], zeros beyond the clip's ends ("shift.conv.weight" [C, 1, 3]:
 *   learned; the shift pattern is only its initial value).  o is conv2's input.
 * State-dict keys, the TSN module's: "base_model.{conv1, bn1}.*", "base_model.conv1_5.*", "base_model.resnext_layer1.B.*",
 * "base_model.layer1_bak.B.*", "base_model.layerL_bak.B.*" with ".mse.*" and ".shift.conv.weight", "new_fc.{weight, bias}".
 * "base_model.conv1_temp.{weight, bias}" is in every checkpoint and unused by the forward: accepted and ignored, as every
 * ".num_batches_tracked" is.
 *
 * depths: blocks per stage, (3, 4, 6, 3) for the model; resnext_layer1 has depths[0] blocks.
 * Legal between tsm_create and the first tsm_set_tensor, later TSM_ERR_INVALID_ARG (as is depths == NULL or a non-finite alpha /
 * beta).  TSM_ERR_UNSUPPORTED: a dtype other than TSM_DTYPE_F32, is_shift != 0 (TDN has no TSM shift), num_segments < 2, height or
 * width not a multiple of 32 or below 64 (a layer4 mSE map could not be pooled), a depth outside 1 .. 64, and after
 * tsm_set_backbone, tsm_set_bottleneck_width, tsm_set_shift_place, tsm_set_non_local(e, 1), tsm_set_temporal_pool(e, 1) or
 * tsm_set_convnext; those six are TSM_ERR_UNSUPPORTED in turn on a TDN engine.  tsm_set_consensus stays legal.
 * tsm_forward / tsm_forward_features / tsm_forward_tap take TSM_LAYOUT_NTCHW, 15 planes per segment, host or device memory, or
 * TSM_LAYOUT_TDN_POOL (below); any other layout: TSM_ERR_UNSUPPORTED.  Everything else is tsm_forward's contract word for word: tsm_tune covers every conv
 * of the engine (conv1_5 runs on conv_igemm as a 1x1 GEMM over patch rows of K = 1024, 588 of them real), tile codes never change
 * a result bit, after tuning the call only enqueues and is capture-safe, and the tune-cache key carries " tdn<depths>".
 * The front end runs in chunks of at most 8 clips through one patch buffer; a clip's result does not depend on the chunking.
 * Launches between conv1 and conv2 of a BottleneckShift: mse_squeeze_kernel and mse_excite_shift_kernel are the only readers of
 * conv1's output, and o is the only full-width tensor written: b, d, s2 and m have r channels, g never reaches memory.
 * Taps (tsm_forward_tap): "diff.conv1_5" (x_c5), "diff.stem" (xd0), "resnext_layer1.B", "stem", "fuse1", "layer1.B", "fuse2",
 * "layerL.B", "layerL.B.conv1", "layerL.B.mse.fwd" / ".mse.bwd" (m+ / m-, [N, H, W, r]), "layerL.B.shift" (o), "layerL.B.conv2".
 *
 * TSM_LAYOUT_TDN_POOL: the 15 planes of a segment are not handed over but FOUND.  `clips` is a tsm_tdn_pool in host memory; it is
 * read during the call, its values travel as kernel parameters and nothing of it is dereferenced later.  `frames` is a pool of
 * transformed frames [n_frames, 3, H, W] fp32 in device memory -- what tsm_preprocess writes as TSM_LAYOUT_NTCHW -- and plane pl
 * of segment s is channel pl % 3 of pool frame frame_of(s, pl / 3).  tdn_front_pool_kernel takes tdn_front_kernel's place in the
 * "diff.front" slot (same arithmetic, same bits as an NTCHW forward of the gathered planes); everything behind it is unchanged.
 *   mode 0 (table): frame_of(s, j) = index[s * 5 + j], `index` int32 [n_clips, T, 5] in device memory, read on the device when the
 *     kernel runs (at replay, for a captured call).  The kernel is total in the table: an entry outside [0, n_frames) reads
 *     nothing and stands for a plane of 0.0f.
 *   mode 1 (window): no table.  Segment k of clip c (counted from first_clip) has centre clip_step * c + clip_stride * k; frame j
 *     is clamp(centre - 2 + j, 0, total_frames - 1) - first_source_frame.  A centre >= total_frames, or a result outside
 *     [0, n_frames), takes pad_frame -- the pool's transformed zero frame, so the differences are exactly zero; a pad_frame
 *     outside [0, n_frames) stands for planes of 0.0f.
 * TSM_ERR_UNSUPPORTED: the layout on an engine without tsm_set_tdn.  TSM_ERR_INVALID_ARG: TSM_MEM_HOST; a struct_size other than
 * sizeof(tsm_tdn_pool); frames NULL or not 8-byte aligned; n_frames <= 0; a mode other than 0 or 1; mode 0 with index NULL; mode 1
 * with clip_step <= 0, clip_stride <= 0 or total_frames <= 0.  Nothing is launched on a refusal.  The first call of a bucket
 * tunes exactly as an NTCHW call does (on the pool it was given); after tuning the call only enqueues and is capture-safe.
 *
 * THE FORWARD IN TWO PHASES.  Everything in front of fuse2 is computed per segment and never looks at a neighbouring segment; only
 * fuse2 onward mixes the segments of a clip.  The two layouts below cut the forward at that seam, so that a segment shared by
 * overlapping clips (or kept between the steps of a live stream) is computed once.  Every kernel keeps one summation order per
 * output whatever the batch: segment phase + trunk phase give the bits of the whole forward on the same frames.
 *   TSM_LAYOUT_TDN_SEGMENTS (segment phase): `clips` is a tsm_tdn_segments in host memory, n_clips counts SEGMENTS, 1 .. max_clips *
 *     T; `logits` is ignored and may be NULL.  Segment i reads pool frames index[5 i .. 5 i + 4] (mode 0) or has centre clip_stride *
 *     (first_clip + i) (mode 1: tdn_front_pool_kernel with T = 1 and clip_step = clip_stride).  Launches: the chunked diff.front +
 *     diff.conv1_5, diff.maxpool, conv1, fuse1 and the blocks of resnext_layer1 and layer1, whose last blocks write straight to
 *     out_d [n, H / 8, W / 8, 256] and out_a [n, H / 4, W / 4, 256]: no fuse2, nothing behind it, no copy.  Taps: the names up to
 *     "layer1.B"; "fuse2" and later are TSM_ERR_INVALID_ARG.  tsm_forward_features is TSM_ERR_UNSUPPORTED.
 *   TSM_LAYOUT_TDN_RING (trunk phase): `clips` is a tsm_tdn_ring in host memory; `table` is int32 [n_clips, T] in device memory, read
 *     on the device when the kernel runs (at replay, for a captured call).  One tdn_fuse_ring_kernel launch takes the fuse2 slot:
 *     x[c, k] = alpha ring_a[slot] + beta up(ring_d[slot]), slot = table[c * T + k], into the trunk's own buffer -- tdn_fuse_kernel's
 *     expression on the gathered operands, bit for bit, moving the bytes fuse2 moves; it is total in the table: a slot outside
 *     [0, n_slots) reads nothing and stands for zeros.  Then layers 2 - 4 and the head (or the feature rows, or a tap) as in a whole
 *     forward.  Taps: "fuse2" onward; earlier names are TSM_ERR_INVALID_ARG.
 * Both: TSM_ERR_UNSUPPORTED on an engine without tsm_set_tdn; TSM_ERR_INVALID_ARG for TSM_MEM_HOST, a struct_size other than the
 * struct's, a NULL pointer, frames not 8-byte aligned, out_a / out_d / ring_a / ring_d not 16-byte aligned, table not 4-byte
 * aligned, n_slots <= 0, a segment count of 0 (TSM_ERR_CAPACITY above max_clips * T) and tsm_tdn_pool's refusals; nothing is
 * launched on a refusal.  The descriptors are read during the call and never dereferenced later.  Timing slots keep those of a whole
 * forward: the launches a phase does not make are "not recorded".  Tuning: the first call of a bucket tunes inside the call, the
 * convs of its own phase only, after which the call only enqueues and is capture-safe.  The phases keep tile codes of their own,
 * apart from whole forwards' (whose buckets are tuned once, all convs): a segment-phase bucket is keyed by the power-of-two bucket
 * of its FRAME count (= segments) plus 2^28, a trunk-phase bucket by bucket(n_clips) * T frames plus 2^29; tsm_conv_tiles reports
 * whole forwards' buckets only. */
int tsm_set_tdn(tsm_engine *e, const int32_t depths[4], float alpha, float beta);

/* Hand one state-dict tensor to the engine (host memory, float32, torch layout: conv OIHW,
 * BN vectors [C], fc [num_class, 2048] -- [num_class, 512] for resnet18 / resnet34).  Names are the reference's TSM.state_dict() keys, e.g.
 * "base_model.layer1.0.conv1.net.weight" ("...conv1.weight" is accepted too).  The engine copies;
 * the caller keeps ownership.  Unknown names return TSM_ERR_INVALID_ARG.  ndim <= 5 (the non-local block's conv3d weights). */
int tsm_set_tensor(tsm_engine *e, const char *name, const float *host_data, const int64_t *shape,
                   int32_t ndim);
/* Fold BatchNorm into the convs, pack to K-major NHWC tiles, upload, allocate the workspace. */
int tsm_finalize(tsm_engine *e);

/* Hot path ---------------------------------------------------------------------------------
 * clips:  n_clips x T x 3 x H x W float32 in `layout`, in `memkind` memory.
 * logits: float32 [n_clips, num_class] in the same memkind.  Raw scores (before softmax).
 *         An identity engine (tsm_set_consensus(e, 1)) writes n_clips * num_segments * num_class floats, ordered
 *         [clip][segment][class]: the caller's buffer must hold that many. */
int tsm_forward(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips,
                float *logits, void *stream);

/* Frame embeddings: tsm_forward with the head replaced by ONE pool_feat_kernel launch -- the reference's classifier-free
 * route, utils/common.py:79-116 (a ResNet with num_classes=0 over every frame, the pooled vector per frame).
 * features: float32 [n_clips * num_segments, feat_dim] in the same memkind (feat_dim = 2048; 512 for resnet18 / resnet34):
 *           row f = mean over the pixels of frame f's last block output when normalize == 0, that row divided by its
 *           Euclidean norm (a norm of 0 counts as 1: an all-zero row stays all-zero, sklearn.preprocessing.normalize)
 *           otherwise.  A frame's pooled value is the avg head's d_pooled to the bit.
 * Everything else is tsm_forward's contract word for word: the first call of a bucket tunes (the tune cache and the tile
 * choices are shared with tsm_forward; no conv launch differs), later calls only enqueue and are capture-safe, n_clips <=
 * max_clips, TSM_MEM_HOST copies and synchronises.  Legal on any finalized engine whatever its consensus, backbone, shift
 * placement or dtype (a shifted engine yields shift-aware per-frame embeddings); the pool launch takes the head's timing
 * slot. */
int tsm_forward_features(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips,
                         float *features, int32_t normalize, void *stream);

/* Tune the kernels of the bucket `n_clips` falls into NOW (synchronous: a few hundred ms of timed launches on the
 * engine's own zeroed input buffer; no caller memory is touched), or read the choices from the tune cache file: what
 * the first tsm_forward of that bucket would otherwise do inside the call.  A no-op when the bucket is already tuned or
 * TSM_AUTOTUNE=0.  Call it at start-up -- a service before it takes requests, a dataset job while its first frames are
 * still being decoded (workoutdetector_amd/inference_count.py does) -- for every batch size that will occur; every
 * tsm_forward(TSM_MEM_DEVICE) afterwards only enqueues.
 * Tune cache: TSM_TUNE_CACHE=<file>, default $XDG_CACHE_HOME/tsm_hip/tune_cache.txt (else ~/.cache/tsm_hip/...); lines
 * are keyed by ABI, library build, device, geometry and dtype, so a second process (or the other ranks of a job) skips
 * the timing pass; TSM_TUNE_CACHE= (empty), 0 or off disables the file. */
int tsm_tune(tsm_engine *e, int32_t n_clips, void *stream);

/* Same as tsm_forward but stops after `stage` and returns that activation (NHWC fp32) in
 * `out` (capacity in floats); shape [N*T, H, W, C] written to out_shape[4].
 * Stages: "input" (packed NHWC4), "conv1" (stem conv+bn+relu), "stem" (after maxpool),
 * "layer{1..4}.{b}" (block output), "layer{L}.{b}.conv1|conv2" (branch intermediates; a BasicBlock has
 * "layer{L}.{b}.conv1" only, its conv2 output is the block output). */
int tsm_forward_tap(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout,
                    int32_t n_clips, const char *stage, float *out, int64_t out_capacity,
                    int64_t out_shape[4], void *stream);

/* Kernel time of the most recent tsm_forward on this engine, measured with HIP events on the
 * stream the kernels ran on (ms); negative if none.  Synchronises on the stop event. */
float tsm_last_forward_ms(tsm_engine *e);

/* Per-launch timing for bench.py's roofline: keep HIP-event pairs around the kernel launches of the
 * next `n_forwards` tsm_forward calls (0 switches it off; at most 64 are kept).  `only_conv3x3` != 0
 * limits the pairs to the 3x3 convolutions (the dominant kernel), which keeps the marker overhead
 * inside a timed region below 0.5 %; launches without a pair report -1.  tsm_layer_times
 * synchronises on forward `forward_index` (0-based since the last tsm_set_layer_timing) and writes
 * one duration in ms per launch, in launch order: pack_input, conv1 (stem), maxpool, then per block
 * [downsample,] conv1, conv2, conv3 (BasicBlock: [downsample,] conv1, conv2), then head (pool + fc).
 * A TDN engine (tsm_set_tdn): per front-end chunk the engine's capacity holds (ceil(max_clips / chunk), chunk = min(8, max_clips,
 * what keeps a chunk's patch rows below 2^29 floats)) diff.front.<i>, diff.conv1_5.<i> -- a forward of fewer chunks leaves the
 * rest not recorded --, then diff.maxpool, conv1 (the stem with its fused max-pool), fuse1; per block of resnext_layer1
 * [downsample,] conv1, conv2, conv3; per block of layer1 the same; fuse2; per BottleneckShift of layers 2 - 4 [downsample,] conv1,
 * mse_squeeze, mse_diff, mse_s2, mse_mix, mse_excite_shift, conv2, conv3; then head.
 * *n_out = number of launches. */
int tsm_set_layer_timing(tsm_engine *e, int32_t n_forwards, int32_t only_conv3x3);
int tsm_layer_times(tsm_engine *e, int32_t forward_index, float *ms_out, int32_t cap, int32_t *n_out);

/* Conv tile code the engine's autotuner chose for each conv launch of an `n_clips` forward, in launch order (stem,
 * then per block [downsample,] conv1, conv2, conv3 -- BasicBlock: [downsample,] conv1, conv2): 1 = 128x128, 2 = 128x64, 3 = 64x64, 4 = 32x32 (one wave),
 * 5 = 128x128 on 8 waves, 6 = 256x256 LDS-DMA kernel (bf16), 7 = weight-stationary 3x3 (bf16, 64 -> 64 / 128 -> 128
 * channels), 8 = the 256x256 kernel run persistently over a workgroup's tiles (bf16, K >= 128), 0 = not tuned (heuristic); + 256 = split-K form of a segmented fp32 layer (one workgroup per tile and K
 * segment, combined in segment order); + 512 = tail split of a segmented 64x64 fp32 layer (only the tiles of the last, partly
 * filled round of resident workgroups run split-K); + 1024 (on conv2's code) = the block runs conv2 + conv3 + residual as ONE
 * launch (conv3's slot is then not used); + 2048 (on conv1's code) = the WHOLE block -- shift, conv1, conv2, conv3 (+ the fused
 * downsample branch) + identity -- runs as ONE launch (bf16 layer1; the conv2 / conv3 slots are then not used); + 4096 (on
 * conv3's code) = that launch also runs the temporal shift + conv1 of the NEXT block (bf16 layer2 / layer3; the next block's
 * conv1 slot is then not used); + 8192 (on conv1's code) = that launch also runs the block's stride-2 conv2 (bf16 layer2.0;
 * conv2's slot is then not used).
 * The report is what an `n_clips` forward RUNS: a fusion bit (1024 / 2048 / 4096 / 8192) is set only where the tuner chose
 * that form and it runs at this clip count; a form forced through the environment (TSM_FUSE_* = 1) is not a tuner choice
 * and sets no bit.
 * The first tsm_forward with a new power-of-two bucket of n_clips
 * times every valid code per layer once, SYNCHRONOUSLY (see Conventions: not capture-safe, a few hundred ms; results are
 * bit-identical across codes); TSM_AUTOTUNE=0 in the environment at tsm_create disables it, TSM_TUNE_CACHE=<file> lets a
 * later process (or the other ranks of a job) read the choices instead of timing again.  Every TSM_* environment
 * variable is read once, in tsm_create. */
int tsm_conv_tiles(tsm_engine *e, int32_t n_clips, int32_t *tiles_out, int32_t cap, int32_t *n_out);

/* Per-op entry points (device pointers; used by the parity tests and as building blocks) ----- */

/* NHWC temporal shift, x/y: [n_frames, hw, c]; n_frames % n_segment == 0; c % (4*fold_div)==0 */
int tsm_temporal_shift(const float *x, float *y, int64_t n_frames, int32_t n_segment, int64_t hw,
                       int32_t c, int32_t fold_div, void *stream);

/* y = act( conv(x, w) * bn_scale + bn_bias [+ residual] ), NHWC.
 * x [n,hi,wi,cin]; w OIHW [cout,cin,k,k] (device, raw); gamma/beta/mean/var [cout] (device);
 * k in {1,3,7}; pad = k/2; residual (nullable) and y [n,ho,wo,cout].
 * shift_segments > 0 applies the temporal shift (fold_div) to x on the fly: k == 1 at stride 1, or k == 3 at stride 1 or
 * 2 (the shift is fused into the conv's loader either way; not combined with a residual).
 * dtype: any tsm_dtype (x / residual / y stay fp32 NHWC at this boundary and are converted to and from
 * the storage format of that dtype around the kernel).
 * Packs the weights on every call: a test/debug entry point, not the fast path.  It has no engine, so it is the one
 * place that reads tuning variables from the environment PER CALL: TSM_CONV_TILE (force a tile shape where valid) and
 * TSM_STEM_DIRECT (bf16-format stems on the generic kernel); neither changes a result bit. */
int tsm_conv_bn_act(const float *x, const float *w, const float *gamma, const float *beta,
                    const float *mean, const float *var, const float *residual, float *y,
                    int32_t n, int32_t hi, int32_t wi, int32_t cin, int32_t cout, int32_t k,
                    int32_t stride, int32_t relu, int32_t shift_segments, int32_t fold_div,
                    int32_t dtype, void *stream);

/* Everything tsm_conv_bn_act takes, plus the conv forms of the engine it cannot reach: block placement's shifted identity,
 * the K-concatenated conv3 + downsample GEMM (a second source), a tile code and the tile walk direction.  Zero-initialise
 * it and set struct_size = sizeof(tsm_conv_args); a zero field keeps tsm_conv_bn_act's meaning. */
typedef struct tsm_conv_args {
  int32_t struct_size;     /* = sizeof(tsm_conv_args), ABI guard                                                      */
  const float *x;          /* [n,hi,wi,cin]                                                                            */
  const float *w;          /* OIHW [cout,cin,k,k], raw                                                                 */
  const float *gamma, *beta, *mean, *var;   /* [cout]                                                                  */
  const float *residual;   /* nullable [n,ho,wo,cout]                                                                  */
  float *y;                /* [n,ho,wo,cout]                                                                           */
  int32_t n, hi, wi, cin, cout, k, stride, relu;
  int32_t shift_segments;  /* T > 0: temporal shift over T segments, fold = channels of the shifted tensor / fold_div   */
  int32_t fold_div;
  int32_t dtype;           /* tsm_dtype                                                                                */
  int32_t shift_target;    /* 0: shift x (as tsm_conv_bn_act).  1: shift the identity -- the residual if given, else the
                              second source -- or, for a 1x1 at stride 2 with neither, x (BasicBlock downsample)         */
  /* Second source (1x1 main conv only, no residual): y = act(conv(x, w) + bn + conv1x1(x2 at stride2, w2) + bn2), one GEMM
   * over K = [cin | cin2] with the summed bias.  x2 [n,hi2,wi2,cin2]; w2 OIHW [cout,cin2,1,1]; the second conv's output
   * size must equal the first's.  x2 == NULL: single source. */
  const float *x2;
  const float *w2;
  const float *gamma2, *beta2, *mean2, *var2;
  int32_t cin2, hi2, wi2, stride2;
  int32_t code;            /* tile code as in tsm_conv_tiles (tile | 0x80 position-major 3x3 | 0x100 split-K | 0x200 tail split); 0 = heuristic.
                              A code that does not fit the launch falls back as in the engine: tsm_launch_trace shows what ran.
                              | 0x4000 (TSM_CONV_CODE_SEGMENTED, this entry point only; no tsm_conv_tiles code carries it): a
                              single fp32 source accumulates K in the engine's segments of ~16 K-steps, as its long-K layers do
                              (a 1x1 at cin >= 1024, an unshifted 3x3 at cin >= 128), so that 0x100 / 0x200 apply
                              to it.  Refused (TSM_ERR_INVALID_ARG), never ignored, where no segmented kernel exists: a
                              residual, a shifted 3x3, the stem, a non-fp32 dtype, a second source (segmented by its whole K
                              already) or fewer than 32 K-steps */
  int32_t reverse;         /* walk the output tiles from the last one to the first                                     */
} tsm_conv_args;
#define TSM_CONV_CODE_SEGMENTED 0x4000

/* One conv launch as the engine makes it (test / debug entry point: packs the weights and allocates on every call; the
 * split forms' segment scratch too).  Refusals come before any launch: TSM_ERR_INVALID_ARG for a shift_target of 1 with
 * nothing to shift, a second source with a residual, 2 * fold above the shifted tensor's channels, n % T != 0 or mismatched
 * sizes; TSM_ERR_UNSUPPORTED for a second source with k != 1 or a fold the dtype's channel groups cannot split (fp32: fold % 4,
 * bf16 formats: fold % 8); TSM_ERR_CAPACITY, as tsm_create, for sizes beyond the kernels' 32-bit indices: n * ho * wo output
 * rows, or the elements of the input, the output, the second source or the packed weights, at or above 2^31, or a padded K
 * that does not fit an int.  tsm_conv_bn_act is this call with the tile of TSM_CONV_TILE as its code. */
int tsm_conv_op(const tsm_conv_args *a, void *stream);

int tsm_maxpool3x3s2(const float *x, float *y, int32_t n, int32_t hi, int32_t wi, int32_t c,
                     void *stream);

/* Fused test transform on the GPU (device pointers), the pre-step of the hot path:
 *   build_test_transform(person_crop=False) = ConvertImageDtype -> Resize(resize) -> CenterCrop(crop)
 *   -> Normalize(ImageNet)            workoutdetector/datasets/build.py:131-136
 * frames: [n, h, w, 3] decoder layout, TSM_PIXEL_U8 or TSM_PIXEL_F32 (values 0..255).
 *         or [n, 3h/2, w] bytes with a TSM_PIXEL_NV12_* code (tsm_pixel): h, w the luma size, both even (an odd side is
 *         TSM_ERR_INVALID_ARG, nothing launched), `frames` 2-byte aligned.  Or frames of another YUV code (tsm_pixel: the
 *         frame size, parity and alignment of each format; a frame that does not fit is TSM_ERR_INVALID_ARG, nothing launched).
 * out:    out_layout TSM_LAYOUT_NTHWC4 -> [n, crop, crop, 4] fp32, TSM_LAYOUT_NTHWC8S -> split-bf16 /
 *         TSM_LAYOUT_NTHWC8B -> bf16 pixel pairs [n, crop, ceil(crop/2), 8] (feed tsm_forward of an engine
 *         of the matching dtype directly) or TSM_LAYOUT_NTCHW -> [n, 3, crop, crop] fp32.
 * scale_255 = 0 reproduces the reference's inference_dataset, which never divides by 255
 * (utils/inference_count.py:412-414); 1 scales to [0,1] first. */
int tsm_preprocess(const void *frames, int32_t pixel, int32_t n, int32_t h, int32_t w, float *out,
                   int32_t out_layout, int32_t resize, int32_t crop, int32_t scale_255, void *stream);

/* The clip iterator of the dataset loop on the GPU (device pointers), between tsm_preprocess and tsm_forward:
 *   for i in range(0, len(video), 8): clip = video[i:i + 16:2], the tail zero-padded   utils/inference_count.py:411-414
 * over TRANSFORMED frames: the buffer `frames` [n_frames, frame_bytes] (any tsm_preprocess layout; rows are opaque) holds
 * every clip_stride-th frame of the video from source frame clip_stride * first_frame on, i.e. buffer frame j = source
 * frame clip_stride * (first_frame + j).  out [n_clips, n_segment, frame_bytes]:
 *   out[c][k] = source frame clip_step * (first_clip + c) + clip_stride * k   if that index < total_frames,
 *               buffer frame pad_frame                                         otherwise (the transformed zero frame).
 * Every index is validated on the host before the launch (TSM_ERR_INVALID_ARG, nothing launched): frame_bytes % 16 == 0,
 * clip_step % clip_stride == 0, each clip starts inside the video, all frames it reads lie in the buffer, and -- when the
 * range has a padded tail -- pad_frame lies in the buffer and is NOT one of the frames the range reads as video frames.
 * n_clips is not limited by the launch geometry: ranges of more than 65535 (clip, segment) rows are cut into several
 * launches inside the call. */
int tsm_gather_clips(const void *frames, int64_t n_frames, int64_t frame_bytes, int64_t first_frame, int64_t total_frames,
                     int64_t pad_frame, int64_t first_clip, int32_t n_clips, int32_t n_segment, int32_t clip_step,
                     int32_t clip_stride, void *out, void *stream);

/* The person-crop test transform fused with the clip iterator (device pointers), straight from staged RAW frames to the
 * input of tsm_forward in ONE launch; the transformed frames are never written:
 *   build_test_transform(person_crop=True) = ConvertImageDtype -> PersonCrop -> Resize((224, 224)) -> Normalize(ImageNet)
 *   datasets/build.py:123-129, datasets/transform.py:226-259 -- from the detector's box on; the Faster-RCNN detector is not
 *   part of this library, the boxes are the caller's.
 * frames: [n_frames, h, w, 3] TSM_PIXEL_U8 or TSM_PIXEL_F32 (values 0..255), tsm_gather_clips' convention: buffer frame j =
 *         source frame clip_stride * (first_frame + j).  Or NV12 frames of 3 h w / 2 bytes (a TSM_PIXEL_NV12_* code, h and w
 *         even, `frames` 2-byte aligned) or of another YUV code (tsm_pixel); the box is in luma pixels and a tap outside the
 *         frame is RGB 0, not a YUV value.
 * boxes:  DEVICE int32 [n_clips, 4] = (top, left, bh, bw) in source-frame pixels, row c for clip first_clip + c.
 * out:    [n_clips, n_segment, ...one frame] in out_layout, as tsm_preprocess with `size` in place of `crop`.
 *   out[c][k] = source frame s = clip_step * (first_clip + c) + clip_stride * k, cropped to box c, resized to size x size
 *   (bilinear, align_corners=False, no antialias, aspect ratio not kept), then (v [/ 255] - mean) / std.  Three rules:
 *   - zero fill: where the box leaves the frame the crop reads 0 (torchvision's tensor crop pads BEFORE Normalize), so a
 *     pixel wholly outside is (0 - mean) / std;
 *   - no person: bh <= 0 or bw <= 0 stands for the whole frame (0, 0, h, w) (transform.py:254, `if w * h == 0: return images`);
 *   - padded tail: s >= total_frames is the reference's zero frame, every channel (0 - mean) / std; nothing is read for
 *     it and the buffer holds no pad frame.
 * Validated on the host before the launch (TSM_ERR_INVALID_ARG, nothing launched), by tsm_gather_clips' rules: non-NULL
 * pointers, positive sizes, pixel type and layout, clip_step % clip_stride == 0, each clip starts inside the video, every
 * source frame < total_frames the range reads lies in [first_frame, first_frame + n_frames).  The BOXES cannot be validated
 * (device memory): the kernel is total in them -- for any int32 contents it reads only inside `frames` (coordinate sums in
 * 64 bits, a tap is read only where it lies in the frame) and writes exactly `out`.  n_clips is not limited by the launch
 * geometry.  Enqueues on `stream`; no synchronisation. */
int tsm_preprocess_clips(const void *frames, int32_t pixel, int64_t n_frames, int32_t h, int32_t w, int64_t first_frame,
                         int64_t total_frames, int64_t first_clip, int32_t n_clips, int32_t n_segment, int32_t clip_step,
                         int32_t clip_stride, const int32_t *boxes, float *out, int32_t out_layout, int32_t size,
                         int32_t scale_255, void *stream);

/* The centre-crop test transform through a DEVICE index table (device pointers), straight from staged RAW frames to the
 * input of tsm_forward in ONE launch -- the access pattern of the reference's FrameDataset (datasets/common.py:99-117), which
 * samples 8 frames per labelled segment with sample_frames(total, 8, start, random=False) (datasets/transform.py:16-65):
 * irregular lists (a segment shorter than 8 frames repeats frames, two segments of one video share no window, unsampled
 * frames are never needed) that the regular windows of tsm_gather_clips / tsm_preprocess_clips cannot express.
 * frames: [n_frames, h, w, 3] TSM_PIXEL_U8 or TSM_PIXEL_F32 (values 0..255): whatever frames the caller staged.
 *         Or NV12 frames of 3 h w / 2 bytes (a TSM_PIXEL_NV12_* code, h and w even, `frames` 2-byte aligned), or frames of
 *         another YUV code (tsm_pixel).
 * index:  DEVICE int32 [n_clips * n_segment], buffer-frame numbers.
 * out:    [n_clips, n_segment, ...one frame] in out_layout; out_layout, resize, crop, scale_255 as tsm_preprocess.
 *   out[c][k] = tsm_preprocess' result for buffer frame index[c * n_segment + k] (build_test_transform(person_crop=False):
 *   ATen bilinear, no antialias, centre crop, normalise) -- the same per-pixel code, so the row equals that frame's row from
 *   tsm_preprocess bit for bit.
 * Validated on the host before the launch (TSM_ERR_INVALID_ARG, nothing launched): non-NULL pointers, positive sizes, pixel
 * type and layout, crop no larger than the resized frame -- exactly tsm_preprocess' checks.  The TABLE cannot be validated
 * (device memory): the kernel is total in it.  An entry outside [0, n_frames) -- INT32_MIN and INT32_MAX included -- reads
 * nothing and yields the normalised zero frame, every channel (0 - mean) / std, as tsm_preprocess_clips' padded tail does;
 * a frame address is formed in 64 bits, and only after the range test.  One grid-stride launch: n_clips is not limited by the
 * launch geometry.  Enqueues on `stream`; no synchronisation. */
int tsm_preprocess_indexed(const void *frames, int32_t pixel, int64_t n_frames, int32_t h, int32_t w, const int32_t *index,
                           int32_t n_clips, int32_t n_segment, float *out, int32_t out_layout, int32_t resize, int32_t crop,
                           int32_t scale_255, void *stream);

/* Either test transform over windows of DIFFERENT frame sizes (device pointers), straight from RAW frames to the input of
 * tsm_forward in ONE launch, in batch order -- a step of a stream server (StreamBatcher), whose streams differ in resolution
 * and complete their windows together; with person_crop = 1 the reference's accuracy option on streams.
 * arena:  one device allocation of arena_bytes, 16-byte aligned, holding every window's frames; pixel: TSM_PIXEL_U8 or
 *         TSM_PIXEL_F32 (values 0..255) for the whole launch, or a TSM_PIXEL_NV12_* code: then a window is n_segment
 *         contiguous NV12 frames of 3 h w / 2 bytes, and a descriptor with an odd h or w is invalid (zero frames); or another
 *         YUV code (tsm_pixel): a window is n_segment contiguous frames of that format, and a descriptor whose h or w has
 *         the wrong parity for it is invalid.
 * desc:   DEVICE int32 [n_windows, 8], 16-byte aligned; row c = {off_lo, off_hi, h, w, top, left, bh, bw}:
 *           off = off_hi * 2^32 + (unsigned) off_lo, the byte offset in `arena` of window c's first frame; its n_segment
 *                 frames are contiguous [n_segment, h, w, 3] of `pixel`;
 *           (top, left, bh, bw): the window's person box in source-frame pixels; read with person_crop = 1 only.
 * out:    [n_windows, n_segment, ...one frame] in out_layout; out_layout, scale_255 as tsm_preprocess.
 *   person_crop = 0: out[c][k] = tsm_preprocess' result (resize, crop) for frame k of window c, the Resize / CenterCrop
 *     geometry computed on the device from the window's own h, w in integers -- the same per-pixel code, so the row equals
 *     that frame's row from tsm_preprocess bit for bit.
 *   person_crop = 1: out[c][k] = tsm_preprocess_clips' result (size = crop; `resize` is not used) for that frame under the
 *     window's box, by its rules -- zero fill where the box leaves the frame, bh <= 0 or bw <= 0 = the whole frame -- and the
 *     same per-pixel code: bit for bit that row.
 * Validated on the host before the launch (TSM_ERR_INVALID_ARG, nothing launched): non-NULL pointers, `arena` and `desc`
 * 16-byte aligned, positive sizes, pixel type and layout, person_crop 0 or 1, crop <= resize with person_crop = 0.  The
 * TABLE cannot be validated (device memory): the kernel is total in it.  A descriptor is valid only if off >= 0,
 * off % 16 == 0, 1 <= h, w <= 65535 and off + n_segment * h * w * 3 * (bytes per channel) <= arena_bytes -- and, with
 * person_crop = 0, the crop fits the resized frame; the test is formed in 64 bits without overflow for ANY int32 words
 * (INT32_MIN and INT32_MAX included) before an address exists.  Every row of an invalid window is the normalised zero frame,
 * every channel (0 - mean) / std, and nothing is read for it; the box is total as in tsm_preprocess_clips.  One grid-stride
 * launch: n_windows is not limited by the launch geometry.  Enqueues on `stream`; no synchronisation.
 *
 * person_crop = TSM_WINDOWS_IMAGE: the IMAGE model's transform over the windows -- tsm_preprocess_image's ToPILImage ->
 * Resize(resize) -> CenterCrop(crop) -> ToTensor -> Normalize, Pillow's antialiased 8-bit resample in integers -- a step of
 * ImageStreamBatcher, whose streams differ in resolution and whose every frame is a window of its own (n_segment = 1).
 *   pixel:  TSM_PIXEL_U8, or a TSM_PIXEL_NV12_* code: a frame is 3 h w / 2 bytes with h and w even and is converted tap by tap
 *           with the integer formula of the other NV12 paths.  TSM_PIXEL_F32 and the other YUV codes: TSM_ERR_UNSUPPORTED,
 *           nothing launched (Pillow's path is 8-bit).
 *   desc:   row c = {off_lo, off_hi, h, w, tab_lo, tab_hi, 0, 0}: off as above; tab = tab_hi * 2^32 + (unsigned) tab_lo, the
 *           byte offset in `arena` of the coefficient block of the window's geometry, exactly tsm_preprocess_image's `tables`
 *           for (h, w, resize, crop): [hb][hk] when the width changes, then [vb][vk] when the height does.  Windows of equal
 *           geometry may share one block.  Words 6 and 7 are reserved and not read.
 *   out:    as above; scale_255 must be 0 and crop <= resize, else TSM_ERR_INVALID_ARG.  A crop whose row of 3 * crop bytes
 *           does not fit 64 KB of LDS: TSM_ERR_UNSUPPORTED.
 *   A descriptor is valid only if the frame conditions above hold (for NV12: both sides even), the crop window lies in the
 *   resized frame, the block -- crop * (2 + ksx) words if the width changes plus crop * (2 + ksy) if the height does, ksx =
 *   2 * max(ceil(w / nw), 1) + 1 and ksy likewise, a count that follows from the geometry alone -- is empty or has tab >= 0,
 *   tab % 16 == 0 and tab + 4 * words <= arena_bytes, and one output row's vertical support fits the kernel's 64 KB of LDS;
 *   all formed in 64 bits for ANY int32 words before an address exists.  An invalid window reads nothing and is the
 *   normalised zero frame.  The table CONTENTS cannot be validated: every bound is clamped before use, as in
 *   tsm_preprocess_image, so the kernel reads only inside the window's frames and its block and writes exactly `out`.
 *   Row (c, k) of a valid window equals, bit for bit, tsm_preprocess_image's row for that frame alone in the same out_layout
 *   (NV12: for the frame converted to RGB).  One grid-stride launch over (window, frame, 8 output rows). */
#define TSM_WINDOWS_IMAGE 16
int tsm_preprocess_windows(const void *arena, int64_t arena_bytes, int32_t pixel, const int32_t *desc,
                           int32_t n_windows, int32_t n_segment, int32_t person_crop, float *out,
                           int32_t out_layout, int32_t resize, int32_t crop, int32_t scale_255, void *stream);

/* feat [n_clips*T, hw, c] NHWC -> logits [n_clips, num_class]; fc_w [num_class, c], fc_b.  Enqueues on `stream`; no
 * synchronisation: the pooled rows between its two launches are a stream-ordered allocation (hipMallocAsync / hipFreeAsync on
 * `stream`), inside a stream capture the graph's own allocation and free nodes. */
int tsm_head(const float *feat, const float *fc_w, const float *fc_b, float *logits,
             int32_t n_clips, int32_t n_segment, int32_t hw, int32_t c, int32_t num_class,
             void *stream);

/* The per-segment head: feat [n_frames, hw, c] NHWC fp32 -> logits [n_frames, num_class] = fc(mean_hw feat[f]) + fc_b, one
 * launch, no scratch (the consensus_type='identity' head; a frame's pooled value is tsm_head's to the bit).
 * c % 8 == 0 and c <= 2048, else TSM_ERR_UNSUPPORTED.  Enqueues on `stream`; no synchronisation. */
int tsm_head_segments(const float *feat, const float *fc_w, const float *fc_b, float *logits, int32_t n_frames,
                      int32_t hw, int32_t c, int32_t num_class, void *stream);

/* The pool of tsm_forward_features on its own (device pointers): feat [n_frames, hw, c] NHWC fp32 -> pooled [n_frames, c] =
 * mean_hw feat[f] (tsm_head's pooled value to the bit) and unit [n_frames, c] = pooled[f] / ||pooled[f]||2 (a norm of 0
 * counts as 1).  Either output may be NULL, both NULL is TSM_ERR_INVALID_ARG; pointers are 16-byte aligned.  One launch,
 * one workgroup per frame, no scratch; the sum of squares runs in an order that depends on c alone, so a frame's rows do
 * not depend on n_frames or on the frames it shares a launch with.  c % 8 == 0 and c <= 2048, else TSM_ERR_UNSUPPORTED.
 * Inputs are finite.  Enqueues on `stream`; no synchronisation. */
int tsm_pool_features(const float *feat, float *pooled, float *unit, int32_t n_frames, int32_t hw, int32_t c, void *stream);

/* The temporal self-similarity matrix (device pointers)   workoutdetector/utils/common.py:118-143 (plot_sim):
 *   unit [n_total, c] fp32, rows [0, row1) valid and of unit length (tsm_pool_features' / tsm_forward_features' unit rows)
 *   dist [n_total, n_total] fp32: the call writes D[i][j] = clamp(1 - <unit_i, unit_j>, 0, 2) for i in [row0, row1) and
 *   j in [0, row1), D[i][i] = 0 exactly, and the mirror D[j][i] from the same computed value -- scikit-learn's
 *   cosine_distances with X is Y.  Nothing else of dist is touched.  row0 = 0, row1 = n_total is the whole matrix; a video
 *   that spans many batches calls once per batch with that batch's band (as tsm_frame_votes carries its history).
 * Exact-fp32 MFMA, ONE chain over k = 0 .. c - 1 in ascending order per element: a value does not depend on which band, tile
 * or launch computed it, and D == D^T bit for bit.  Rows are not re-normalised: garbage in unit gives garbage distances,
 * but the kernel is total -- for any float contents it reads only unit rows [0, row1) and writes exactly the region above.
 * TSM_ERR_INVALID_ARG (nothing launched): NULL or not 16-byte aligned pointers, row0 < 0, row0 >= row1, row1 > n_total,
 * c <= 0; TSM_ERR_UNSUPPORTED: c % 8 != 0.  No upper limit on c; n_total is not limited by the launch geometry.
 * Enqueues on `stream`; no synchronisation. */
int tsm_cosine_distances(const float *unit, int32_t n_total, int32_t c, int32_t row0, int32_t row1, float *dist, void *stream);

/* The non-local block's two kernels (device pointers, fp32, NHWC; enqueue on `stream`, no synchronisation).
 * tsm_maxpool2x2: MaxPool3d((1, 2, 2)) = a 2x2 max-pool at stride 2, floor mode, no padding, of channels [c0, c0 + c) of
 *   x [n, hi, wi, ld] (ld = the row stride in floats) into the DENSE y [n, hi / 2, wi / 2, c]; a last odd row / column is
 *   dropped.  TSM_ERR_INVALID_ARG: NULL pointers, hi < 2 or wi < 2, c0 / c / ld not multiples of 4, c0 + c > ld, pointers not
 *   16-byte aligned.
 * tsm_nonlocal_attention: y[b, i, :] = sum_j softmax_j(q[b, i, :] . k[b, j, :]) v[b, j, :] for b < n_clips, i < nq, j < nk over
 *   d channels, no scale factor.  Row (b, i) of q starts at q + (b * nq + i) * ldq, row (b, j) of k / v at
 *   (b * nk + j) * ldkv, row (b, i) of y at (b * nq + i) * ldy: the operands may be channel slices of wider tensors.  Online
 *   softmax: no buffer proportional to nq * nk exists.  Every output element is summed in ONE fixed order that depends on
 *   (i, nk) only -- not on the clip, the number of clips or the grid -- without atomics: a clip's rows equal its own
 *   single-clip launch bit for bit.  Rows >= nq and keys >= nk are neither read nor written.
 *   TSM_ERR_UNSUPPORTED (nothing launched): d other than 256 or 512.  TSM_ERR_INVALID_ARG: NULL pointers, non-positive sizes,
 *   a row stride below d, ldq or ldkv not a multiple of 4, q / k / v not 16-byte aligned, n_clips > 65535, nk > 2^31 - 65. */
int tsm_maxpool2x2(const float *x, int64_t ld, int32_t c0, int32_t c, float *y, int32_t n, int32_t hi, int32_t wi, void *stream);
int tsm_nonlocal_attention(const float *q, int64_t ldq, const float *k, const float *v, int64_t ldkv, float *y, int64_t ldy,
                           int32_t n_clips, int32_t nq, int32_t nk, int32_t d, void *stream);

/* Scores -> states on the GPU (device pointers), the post-step of the hot path:
 *   logits [n_clips, num_class] fp32 -> states [n_clips] int32: (softmax != 0: fp32 softmax over the classes,) the FIRST
 *   maximum, its class id if the score >= threshold, else -1; top_score (nullable) [n_clips] receives that score.
 * A streaming consumer (count_by_video_model, utils/inference_count.py:285-339) then copies 4-8 bytes per window to
 * the host instead of the logits and feeds pred_to_count directly. */
int tsm_scores_to_states(const float *logits, int32_t n_clips, int32_t num_class, int32_t softmax, float threshold,
                         int32_t *states, float *top_score, void *stream);

/* The per-frame transform of the reference's IMAGE model on the GPU (device pointers), one launch from staged uint8 frames to
 * the packed input of a num_segments = 1 engine:
 *   data_transform = ToPILImage -> Resize(resize) -> CenterCrop(crop) -> ToTensor -> Normalize(ImageNet)
 *   workoutdetector/utils/inference_count.py:27-34 -- Pillow's ImagingResample for 8-bit channels with the bilinear (triangle)
 *   filter: antialiased (support = max(in / out, 1)), a horizontal pass rounded to uint8, then a vertical pass over those
 *   uint8 values, each u8 = clamp((2^21 + sum(pixel * k)) >> 22, 0, 255) in int32.  NOT tsm_preprocess (ATen's bilinear on
 *   floats without antialias): for a 720 x 1280 frame the two differ by several grey levels per pixel.
 * frames: uint8 [n, h, w, 3].  The channel order is kept as given (the reference hands cv2's BGR frames to ToPILImage as they
 *         are: which order the model was trained on is the caller's business).
 * Sizes:  torchvision's Resize(int): shorter side -> resize, longer -> int(resize * long / short); an axis that keeps its size
 *         is not resampled (Pillow skips that pass).  Crop window: top = int(round((nh - crop) / 2.0)) (round half to even),
 *         left likewise.  Only the window's pixels are computed and only their taps are read.
 * tables: DEVICE int32 [table_words], the coefficient tables the HOST computes in double (Pillow's precompute_coeffs +
 *         normalize_coeffs_8bpc; workoutdetector_amd/transform.py::image_tables builds and caches the block), for the crop
 *         window's output indices only.  When the width changes: hb [crop][2] = (first source column, taps) of output columns
 *         left .. left + crop - 1, then hk [crop][ksx] = their weights, int(w * 2^22 +- 0.5), zero-padded to ksx =
 *         ceil(max(w / nw, 1)) * 2 + 1; when the height changes: vb [crop][2], vk [crop][ksy] likewise for rows top .. top +
 *         crop - 1.  table_words must be exactly crop * (2 + ksx) [+ crop * (2 + ksy)] (0 and tables == NULL when neither axis
 *         changes), else TSM_ERR_INVALID_ARG.  The table CONTENTS cannot be validated (device memory): the kernel is total in
 *         them -- every bound is clamped into the frame before use, so it reads only inside `frames` and writes exactly `out`.
 * out:    as tsm_preprocess: TSM_LAYOUT_NTHWC4 / NTHWC8S / NTHWC8B / NTCHW, values ((u8 / 255) - mean) / std in fp32.
 * One workgroup per (frame, band of <= 8 output rows) keeps the horizontally resampled rows under the band's vertical support
 * in LDS; TSM_ERR_UNSUPPORTED (nothing launched) when one output row's support does not fit 64 KB (crop 224: beyond a 47x
 * vertical downscale; a 2160-line frame to 256 is 8.4x).  Enqueues on `stream`; no synchronisation. */
int tsm_preprocess_image(const void *frames, int32_t n, int32_t h, int32_t w, const int32_t *tables, int64_t table_words,
                         float *out, int32_t out_layout, int32_t resize, int32_t crop, void *stream);

/* The image model's vote on the GPU (device pointers)   workoutdetector/utils/inference_count.py:221-231:
 *   logits [n_frames, num_class] fp32 -> pred [n_frames] int32, the FIRST arg-max of every row (numpy.argmax's tie rule), and
 *   state [n_frames] int32 0 / 1 = (sum of the last up-to-7 preds ending at that frame) >= 4: the reference's deque(maxlen=7)
 *   and `sum(que) >= 4`.  The sum is over CLASS IDS, exactly as the reference's is: with two classes "at least 4 of the last 7
 *   frames are class 1"; with more classes it is whatever that sum gives -- reproduced, not repaired.
 * A video spans many calls: history [n_hist], n_hist in 0..6, holds the preds of the frames before this batch, oldest first;
 * history_out [6] (nullable; must not alias history) receives the last min(6, n_hist + n_frames) preds of (history ++ this
 * batch), oldest first, and -1 in the slots behind them -- the next call's history, with that count.  Inputs are finite (NaN handling is the reference's:
 * unspecified).  One launch, no host synchronisation, on `stream`. */
int tsm_frame_votes(const float *logits, int32_t n_frames, int32_t num_class, const int32_t *history, int32_t n_hist,
                    int32_t *pred, int32_t *state, int32_t *history_out, void *stream);

/* The accuracy tally on the GPU (device pointers)   scripts/eval_classification.py:42-49, its intent (the snapshot compares a
 * logits row with the label and never increments class_total):
 *   logits [n, num_class] fp32, labels [n] DEVICE int32 -> pred [n] int32 (nullable), the FIRST arg-max of every row
 *   (tsm_frame_votes' tie rule), and per class the counters correct [num_class] / total [num_class] (int32), which
 *   ACCUMULATE: for a label in [0, num_class) total[label] += 1 and correct[label] += (pred == label); any other label is
 *   counted nowhere (the kernel is total in the labels).  The caller zeroes the counters once and reads them once per
 *   dataset; correct and total must not alias (TSM_ERR_INVALID_ARG).
 * One launch of one workgroup: per-launch counts in LDS, then one thread per class adds them to the global counters with an
 * ordinary load, add and store -- launches on one stream are ordered, so calls that share counters must share a stream.
 * num_class <= 1024, else TSM_ERR_UNSUPPORTED.  Inputs are finite.  No host synchronisation, on `stream`. */
int tsm_top1_tally(const float *logits, const int32_t *labels, int32_t n, int32_t num_class, int32_t *pred, int32_t *correct,
                   int32_t *total, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* TSM_HIP_H_ */
