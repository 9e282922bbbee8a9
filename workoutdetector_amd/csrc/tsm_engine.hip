// Host engine + C ABI (include/tsm_hip.h) for the TSM-ResNet clip forward on MI355X (ResNet-50 by default; ResNet-18 / 34
// through tsm_set_backbone; the shift in front of conv1 by default, in front of the whole block through tsm_set_shift_place),
// for the ConvNeXt-Base image model through tsm_set_convnext (build_convnext_topology, run_convnext), and for TDN-ResNet50
// through tsm_set_tdn (build_tdn_topology, run_tdn).  Construction is one path for all of them: the topology builders spell
// every tensor once into the engine's manifest (build_manifest), tsm_set_tensor accepts what the manifest names, and
// tsm_finalize checks the manifest, packs every conv by its kind, and allocates the workspace (alloc_workspace).
//
// Owns: packed weights (BatchNorm folded, K-major), an NHWC fp32 activation workspace sized for
// max_clips, one HIP stream, two timing events.  The forward is a fixed schedule of kernel launches
// (csrc/tsm_*.hip, one file per kernel family: tsm_device.h lists them); nothing here falls back to a CPU path.
//
// Reference behaviour mirrored: workoutdetector/models/tsm.py:409-419 (TSM.forward), :125-137
// (shift in front of every block's conv1), :451-473 (state-dict naming); torchvision-0.13
// ResNet-50 v1.5 (stride on conv2, BN eps 1e-5) and ResNet-18 / 34 (BasicBlock: stride on conv1).
#include <hip/hip_runtime.h>

#include <sys/stat.h>

#include <algorithm>
#include <cerrno>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/tsm_hip.h"
#include "tsm_host_util.h"
#include "tsm_kernels.h"

#ifndef TSM_BUILD_ID   // workoutdetector_amd/build.py passes the sha of csrc/; a hand build falls back to its own time stamp
#define TSM_BUILD_ID __DATE__ "/" __TIME__
#endif

namespace {

using namespace tsm_host;

// The tag is also what workoutdetector_amd/build.py looks for in the FILE to decide whether a prebuilt library belongs to
// the tree it sits in (mtimes do not survive a copy to another machine).
const char kBuildTag[] = "tsm-build-id:" TSM_BUILD_ID;

// Backbones by depth: blocks per stage and the block type.  Planes are 64, 128, 256, 512 for all of them; a Bottleneck widens
// its output by 4, a BasicBlock by 1 (torchvision resnet18 / resnet34 / resnet50).  A Bottleneck's mid width is planes *
// width_per_group / 64 (tsm_set_bottleneck_width: 64, or 128 for wide_resnet50_2).
struct Backbone {
  int depth;
  int blocks[4];
  bool basic;
};
constexpr Backbone kBackbones[] = {{18, {2, 2, 2, 2}, true}, {34, {3, 4, 6, 3}, true}, {50, {3, 4, 6, 3}, false}};
constexpr int kPlanes[4] = {64, 128, 256, 512};

const Backbone *find_backbone(int depth) {
  for (const Backbone &b : kBackbones)
    if (b.depth == depth) return &b;
  return nullptr;
}

// Message of the last failure of an engine-less entry point (tsm_create, the per-op functions): per calling thread, so
// two threads driving two engines never write the same string (include/tsm_hip.h, "no global state").
thread_local std::string g_create_error;

struct HostTensor {
  std::vector<float> data;
  std::vector<int64_t> shape;
};

// Which tensors a conv layer reads and how tsm_finalize packs them (build_manifest, pack_conv); wkey = "<name>.weight", a conv
// bias is "<name>.bias" beside it.
enum class ConvKind {
  kBn,         // [cout, cin, k, k] + the BatchNorm `bnp`
  kNlQkv,      // a non-local block's theta | phi | g as one 1x1 conv: three [cout / 3, cin, 1, 1, 1] with a bias, no BatchNorm
  kNlW,        // its W: "<nlp>.W.0" [cout, cin, 1, 1, 1] with a bias + the BatchNorm "<nlp>.W.1"
  kCnxStem,    // a ConvNeXt engine's GEMMs, all with a bias and no BatchNorm: the stem [cout, 3, 4, 4],
  kCnxDown,    // a downsample [cout, cout / 2, 2, 2],
  kCnxFc1,     // fc1 [cout, cin]
  kCnxFc2,     // and fc2 [cout, cin] with the block's gamma folded in
  kTdnBias,    // a TDN engine's conv with a bias in front of its BatchNorm, folded into the BatchNorm's mean
  kTdnConv15,  // conv1_5 [64, 12, 7, 7] (no bias) + BatchNorm, as a 1x1 GEMM over the front end's patch rows
};

struct ConvLayer : LayerGeom {   // cp, kp, kseg: tsm_host_util.h, layer_geometry
  std::string wkey, bnp;
  int cin = 0, cout = 0, k = 1, stride = 1;
  ConvKind kind = ConvKind::kBn;
  std::string nlp;    // (kNlQkv, kNlW) "base_model.layerL.B.nl"
  std::string gkey;   // (kCnxFc2) the block's "gamma"
  float *d_w = nullptr, *d_b = nullptr;
};

// One tensor of the engine's manifest (build_manifest): what tsm_set_tensor accepts under this key and its other spellings,
// and what tsm_finalize requires of it.
struct TensorSpec {
  std::string key;
  std::vector<int64_t> shape;
  std::string missing, mismatch;   // tsm_finalize's refusal when it is absent / has another shape
  bool joins = false;              // checked together with the entry in front of it: all absences of the group first, then the shapes
  bool ignored = false;            // accepted, never read (".num_batches_tracked", TDN's "conv1_temp")
};

struct Block {
  // indices into convs, down = -1 if none.  A Bottleneck has conv1 (1x1, shifted), conv2 (3x3, strided), conv3 (1x1,
  // + identity); a BasicBlock has conv1 (3x3, shifted, strided) and conv2 (3x3, + identity), conv3 = -1.
  int conv1, conv2, conv3, down;
  int stride;
  std::string name;  // "layerL.B"
  // conv3 + downsample as ONE GEMM over K = [conv3 input channels | block input channels]
  float *d_wf = nullptr, *d_bf = nullptr;
  // conv2 + conv3 (+ residual) as ONE kernel (tsm::launch_conv23_fused): fp32 / split-bf16 blocks without a downsample branch whose
  // mid tensor has 64 / 128 channels and conv3 4x as many (layer1.1-2, layer2.1-3), or 128 channels and conv3 2x as many
  // (wide_resnet50_2's layer1.1-2); d_w3f = conv3's folded weights in fragment order
  // (fp32 / split-bf16; the bf16 form, 64 channels only, reads conv3's own packed matrix: d_w3f stays null, cmid = 64)
  float *d_w3f = nullptr;
  int cmid = 0;
  int cout3 = 0;   // conv3's output channels where cmid is set: 4 * cmid, or 2 * cmid (conv23_fused2_kernel)
  // a non-local engine's wrapped blocks: the theta | phi | g conv and the W conv behind the block (-1: not wrapped), and the
  // tap name of the block's OWN output ("layerL.B.block" when wrapped: "layerL.B" is then the wrapper's)
  int nl_qkv = -1, nl_w = -1;
  std::string out_name;
  // the segment count of the block's stage: cfg.num_segments, or half of it from layer2 on in a temporal-pool engine; and
  // whether the temporal pool runs behind this block (the last one of layer1)
  int T = 0;
  bool tpool_after = false;
  // a TDN engine: the block's long-term module between conv1 and conv2 (index into tdn_mse; -1: a plain Bottleneck), and whether
  // the block belongs to the difference path (resnext_layer1, on the maps of xd0) instead of the trunk
  int mse = -1;
  bool diff_path = false;
};

// A TDN engine's long-term module (mSE + the learned temporal conv) of one BottleneckShift: its packed weights on the device
// (tsm_host_util.h: tdn_pack_mse).
struct TdnMse {
  int c = 0;          // conv1's width; the module works on r = c / 16 channels
  std::string key;    // "base_model.layerL_bak.B": its tensors are "<key>.mse.*" and "<key>.shift.conv.weight"
  float *d_wq = nullptr, *d_bq = nullptr, *d_dw = nullptr, *d_k2 = nullptr, *d_b2 = nullptr, *d_k4 = nullptr, *d_b4 = nullptr;
  float *d_w3 = nullptr, *d_b3 = nullptr, *d_wt = nullptr;
};

// A ConvNeXt engine (tsm_set_convnext): one LayerNorm's affine pair, one block, one stage.  Every GEMM is a ConvLayer of
// e->convs (added through add_conv, in launch order: the stem, then per stage [its downsample,] fc1 and fc2 of every block).
struct CnxNorm {
  std::string key;   // "<key>.weight" / "<key>.bias", [c]
  int c = 0;
  float *d_w = nullptr, *d_b = nullptr;
};
struct CnxBlock {
  int c = 0, fc1 = -1, fc2 = -1;   // width; indices into convs
  std::string name;                // "stages.S.blocks.B"
  std::string dwkey;               // "<name>.conv_dw": "<dwkey>.weight" [c, 1, 7, 7] / "<dwkey>.bias"
  CnxNorm norm;
  float *d_dw = nullptr, *d_dwb = nullptr;   // conv_dw [49][c] (cnx_pack_dw) and its bias
};
struct CnxStage {
  int down = -1;   // the 2x2 stride-2 conv as a 1x1 over the space-to-depth rows (-1: stage 0)
  CnxNorm norm;    // the LayerNorm in front of it
  int first = 0, count = 0;   // its blocks in e->cnx_blocks
};

// A device buffer between two poisoned bands (tsm_host_util.h: guard_layout).  tsm_conv_op's temporaries always are; the
// engine's buffers are under TSM_POISON=1.
struct GuardBuf {
  std::string name;
  char *base = nullptr;     // the allocation (what hipFree takes)
  GuardLayout lay;
  size_t elem_bytes = 4;    // for the message: offsets are reported in elements of the buffer
  float *ptr() const { return reinterpret_cast<float *>(base + lay.lead); }
};

// Allocate `payload_bytes` between bands sized for `frame_bytes`, the WHOLE allocation filled with the poison word (so the
// payload too: whatever is not written afterwards stays poison).  Synchronous.
hipError_t guard_alloc(GuardBuf *g, const char *name, size_t payload_bytes, size_t frame_bytes, size_t elem_bytes = 4) {
  g->name = name;
  g->lay = guard_layout(payload_bytes, frame_bytes);
  g->elem_bytes = elem_bytes;
  void *q = nullptr;
  hipError_t st = hipMalloc(&q, g->lay.total());
  if (st != hipSuccess) return st;
  g->base = static_cast<char *>(q);
  st = hipMemsetD32(reinterpret_cast<hipDeviceptr_t>(q), (int)kPoisonWord, g->lay.total() / 4);
  return st != hipSuccess ? st : hipDeviceSynchronize();
}

// Both bands copied to the host (the bands only) and compared with the poison word.  Returns hipSuccess with *msg empty when
// they are intact, with *msg naming buffer, side and element offset when not.
hipError_t guard_verify(const GuardBuf &g, std::string *msg) {
  std::vector<uint32_t> host(std::max(g.lay.lead, g.lay.tail) / 4);
  for (int after = 0; after < 2; ++after) {
    const size_t bytes = after ? g.lay.tail : g.lay.lead;
    const hipError_t st = hipMemcpy(host.data(), g.base + (after ? g.lay.lead + g.lay.payload : 0), bytes, hipMemcpyDeviceToHost);
    if (st != hipSuccess) return st;
    const long bad = guard_first_bad(host.data(), bytes / 4);
    if (bad >= 0) {
      *msg = guard_message(g.name, g.lay, after != 0, (size_t)bad, g.elem_bytes, host[bad]);
      return hipSuccess;
    }
  }
  return hipSuccess;
}

}  // namespace

struct tsm_engine {
  tsm_config cfg{};
  int depth = 50;             // tsm_set_backbone
  int width = 64;             // tsm_set_bottleneck_width: torchvision's width_per_group
  int place = 0;              // tsm_set_shift_place: 0 blockres, 1 block
  int temporal_pool = 0;      // tsm_set_temporal_pool: max-pool over time in front of layer2; layers 2-4 and the head see T / 2 frames per clip
  int non_local = 0;          // tsm_set_non_local: non-local blocks around layer2.{0,2} and layer3.{0,2,4} (fp32 Bottleneck engines)
  int convnext = 0;           // tsm_set_convnext: a ConvNeXt-Base topology (cnx_*) in place of the ResNet one
  int backbone_set = 0;       // tsm_set_backbone / tsm_set_bottleneck_width / tsm_set_shift_place has been called
  int cnx_depths[4] = {0, 0, 0, 0};
  std::vector<CnxBlock> cnx_blocks;
  CnxStage cnx_stages[4];
  CnxNorm cnx_stem_norm, cnx_head_norm;
  int tdn = 0;                // tsm_set_tdn: a TDN-ResNet50 topology; input [n_clips, T, 15, H, W]
  int tdn_depths[4] = {0, 0, 0, 0};
  float tdn_alpha = 0.5f, tdn_beta = 0.5f;
  std::vector<TdnMse> tdn_mse;
  int tdn_chunk = 0;          // clips per front-end chunk (tdn_chunk_clips)
  tsm_tdn_pool tdn_pool{};    // TSM_LAYOUT_TDN_POOL: the caller's descriptor, copied behind its checks, for the running call only
  tsm_tdn_segments tdn_seg{}; // TSM_LAYOUT_TDN_SEGMENTS: the same (its frame fields also go into tdn_pool: tdn_segments_pool)
  tsm_tdn_ring tdn_ring{};    // TSM_LAYOUT_TDN_RING: the same
  int hd = 0, wd = 0;         // the difference path's maps (xd0, resnext_layer1)
  float *d_patches = nullptr; // conv1_5's patch rows of one chunk
  // the long-term module's r-channel maps: b, d+, d-, m+, m- at the block's size; pooled d+, d-, s2+, s2- at half of it
  float *d_mse[9] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  int consensus = 0;          // tsm_set_consensus: 0 avg ([n_clips, num_class]), 1 identity ([n_clips, T, num_class])
  int feat = 2048;            // channels of the last stage = the classifier's input width
  int features = 0;           // for the duration of a tsm_forward_features call: 1 = the forward ends in the pooled rows, 2 = in the unit rows
  bool weights_started = false;   // a tsm_set_tensor call has been made: the backbone is fixed
  size_t tune_sig_base = 0;   // length of tune_sig before the backbone / placement suffix
  std::string err;
  hipStream_t stream = nullptr;
  bool finalized = false;
  int prec = tsm::kPrecF32;
  float *d_tap = nullptr;     // fp32 staging for tsm_forward_tap on split-format engines
  std::map<std::string, HostTensor> tensors;
  std::vector<TensorSpec> manifest;   // every tensor of this topology (build_manifest), in the order tsm_finalize checks them
  std::vector<ConvLayer> convs;
  std::vector<Block> blocks;
  float *d_fcw = nullptr, *d_fcb = nullptr;
  float *d_in = nullptr;      // raw clips staged from host memory
  float *d_in4 = nullptr;     // NHWC4 packed input
  float *buf[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
  float *d_pooled = nullptr, *d_logits = nullptr;
  float *d_partial = nullptr;   // split-K segment sums [segments][M][Cout] (fp32 engines)
  size_t partial_elems = 0;
  size_t buf_elems = 0;
  int h1 = 0, w1 = 0, hp = 0, wp = 0;  // stem conv / maxpool output sizes
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool have_time = false;
  std::vector<void *> allocs;
  // TSM_POISON=1 (read once in tsm_create; tests only): every device buffer sits between poisoned bands, every forward first
  // fills the activation / scratch buffers with the poison word, and after its last launch synchronises and verifies all
  // bands (TSM_ERR_GUARD).  No result bit changes; forwards become synchronous and are not capture-safe.
  bool poison = false;
  std::vector<GuardBuf> guards;
  // per-launch timing (tsm_set_layer_timing): timing[f] = events of forward f, 2 per launch
  // conv tile autotune: per frame count, one ConvTile per conv layer (0 = not tuned yet)
  std::map<int, std::vector<int>> tile_cache;
  bool autotune = true;
  bool stem_pool = true;    // TSM_STEM_POOL=0: separate max-pool launch behind the direct stem
  bool stem_direct = true;  // TSM_STEM_DIRECT=0: bf16-format stems on the generic implicit-GEMM kernel (bit-identical, slower)
  bool stem_planar = true;  // TSM_STEM_PLANAR=0: an NTCHW input is packed by its own launch first (bit-identical, one more pass over the input)
  // TSM_TUNE_CACHE=<file>: tuned tile codes are appended to / read from this file, one line per bucket, keyed by
  // `tune_sig` (ABI, device name, geometry, dtype): a later process skips the timing pass.  Codes never change
  // results and every code is re-validated against its layer at launch (Forward::conv, plan_forward), so a stale, foreign
  // or hand-edited line can only cost speed; malformed lines are ignored.
  std::string tune_path, tune_sig;
  // Tuning hooks, read ONCE in tsm_create (never per launch): TSM_CONV_TILE=<name> forces one tile shape wherever it
  // is valid, TSM_CONV_CODE=<int> one tile code (tile | kCodeSplitK = split-K form); tests and tools/ sweeps only.
  int force_tile = 0, force_code = -1;
  int fuse23 = -1;   // TSM_FUSE_CONV23: 0 never, 1 wherever a block is eligible, unset: the autotuner times both forms
  int fuse_block = -1;   // TSM_FUSE_BLOCK: the same for the whole-Bottleneck kernel (bf16, layer1.1 / layer1.2)
  int fuse31 = -1;       // TSM_FUSE_C3C1: the same for conv3 of block b + shift + conv1 of block b + 1 as one launch (bf16, layer2)
  int fuse_front = -1;   // TSM_FUSE_FRONT: the same for shift + conv1 + the stride-2 conv2 of layer2.0 as one launch (bf16)
  bool pos_major = true; // TSM_POS_MAJOR=0: the tuner does not offer the position-major 3x3 codes (kCodePosMajor); for the A/B
  bool pos_balance = true; // TSM_POS_BALANCE=0: position-major launches keep equal-count XCD runs (ConvParams::pos_balance); for the A/B
  bool tile_64x128 = true; // TSM_TILE_64X128=0: the tuner does not offer the 64x128 tile (kTile64x128); for the A/B
  int walk = -1;         // TSM_WALK: 0 / 1 every tile-walking launch walks forward / in reverse; unset: alternate (Forward::next_dir)
  int n_cu = 256;
  int timing_left = 0;
  bool timing_only3x3 = false;
  std::vector<std::vector<hipEvent_t>> timing;
  std::vector<hipEvent_t> event_pool;
  std::vector<hipEvent_t> *cur_timing = nullptr;
};

namespace {

int fail(tsm_engine *e, int code, const std::string &msg) {
  if (e) e->err = msg; else g_create_error = msg;
  return code;
}

#define TSM_HIP(e, call)                                                                        \
  do {                                                                                          \
    hipError_t _st = (call);                                                                    \
    if (_st != hipSuccess)                                                                      \
      return fail((e), TSM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_st));        \
  } while (0)

// Appends a conv layer in its packed geometry; returns its index.  `segmented` = false keeps a long-K fp32 layer whole-K.
int add_conv(tsm_engine *e, const std::string &wkey, const std::string &bnp, int cin, int cout, int k, int stride, bool segmented,
             ConvKind kind = ConvKind::kBn) {
  ConvLayer c;
  c.kind = kind;
  static_cast<LayerGeom &>(c) = layer_geometry(cin, k, stride, e->prec);
  if (!segmented) c.kseg = 0;
  c.wkey = wkey; c.bnp = bnp; c.cin = cin; c.cout = cout; c.k = k; c.stride = stride;
  e->convs.push_back(c);
  return (int)e->convs.size() - 1;
}

// The ConvNeXt topology (timm 0.5.4 key spelling).  Every GEMM goes through add_conv as a 1x1 conv: the stem over its packed 4x4
// patches (K = 64), a downsample over the space-to-depth rows (K = 4 * C / 2), fc1 (C -> 4 C) and fc2 (4 C -> C, + the block
// input).  Layers without a residual are segmented where their K is long enough, as every such layer of the ResNets is.
void build_convnext_topology(tsm_engine *e) {
  e->convs.clear();
  e->blocks.clear();
  e->cnx_blocks.clear();
  auto norm = [](const std::string &key, int c) { CnxNorm n; n.key = key; n.c = c; return n; };
  add_conv(e, "stem.0.weight", "", kCnxStemK, kCnxWidths[0], 1, 1, true, ConvKind::kCnxStem);
  e->cnx_stem_norm = norm("stem.1", kCnxWidths[0]);
  for (int s = 0; s < kCnxStages; ++s) {
    const int c = kCnxWidths[s];
    const std::string sp = "stages." + std::to_string(s);
    CnxStage &st = e->cnx_stages[s];
    st = CnxStage();
    if (s > 0) {
      st.norm = norm(sp + ".downsample.0", c / 2);
      st.down = add_conv(e, sp + ".downsample.1.weight", "", 4 * (c / 2), c, 1, 1, true, ConvKind::kCnxDown);
    }
    st.first = (int)e->cnx_blocks.size();
    st.count = e->cnx_depths[s];
    for (int b = 0; b < st.count; ++b) {
      CnxBlock blk;
      blk.c = c;
      blk.name = sp + ".blocks." + std::to_string(b);
      blk.dwkey = blk.name + ".conv_dw";
      blk.norm = norm(blk.name + ".norm", c);
      blk.fc1 = add_conv(e, blk.name + ".mlp.fc1.weight", "", c, 4 * c, 1, 1, true, ConvKind::kCnxFc1);
      blk.fc2 = add_conv(e, blk.name + ".mlp.fc2.weight", "", 4 * c, c, 1, 1, false, ConvKind::kCnxFc2);
      e->convs[blk.fc2].gkey = blk.name + ".gamma";
      e->cnx_blocks.push_back(blk);
    }
  }
  e->cnx_head_norm = norm("head.norm", kCnxWidths[kCnxStages - 1]);
  e->feat = kCnxWidths[kCnxStages - 1];
}

// The TDN topology (include/tsm_hip.h, tsm_set_tdn; the TSN module's key spelling).  convs[0] is the trunk's stem, convs[1]
// conv1_5 as a 1x1 GEMM over K = kTdnPatchK; then resnext_layer1's plain Bottlenecks (the difference path), then layer1_bak's
// plain Bottlenecks and the BottleneckShift blocks of layer2_bak .. layer4_bak, each with a TdnMse.  Every conv but conv1_5
// has a bias.
void build_tdn_topology(tsm_engine *e) {
  e->convs.clear();
  e->blocks.clear();
  e->tdn_mse.clear();
  const ConvKind kb = ConvKind::kTdnBias;
  add_conv(e, "base_model.conv1.weight", "base_model.bn1", 3, 64, 7, 2, false, kb);
  add_conv(e, "base_model.conv1_5.0.weight", "base_model.conv1_5.1", kTdnPatchK, 64, 1, 1, true, ConvKind::kTdnConv15);
  for (int li = -1; li < 4; ++li) {   // -1: resnext_layer1
    const int stage = li < 0 ? 0 : li, planes = kPlanes[stage], cout = 4 * planes;
    int cin = stage == 0 ? 64 : 4 * kPlanes[stage - 1];
    for (int b = 0; b < e->tdn_depths[stage]; ++b) {
      const int stride = (b == 0 && stage > 0) ? 2 : 1;
      const std::string lname = li < 0 ? "resnext_layer1" : "layer" + std::to_string(li + 1);
      const std::string p = "base_model." + lname + (li < 0 ? "." : "_bak.") + std::to_string(b);
      Block blk;
      blk.stride = stride;
      blk.T = e->cfg.num_segments;
      blk.name = blk.out_name = lname + "." + std::to_string(b);
      blk.diff_path = li < 0;
      blk.conv1 = add_conv(e, p + ".conv1.weight", p + ".bn1", cin, planes, 1, 1, true, kb);
      blk.conv2 = add_conv(e, p + ".conv2.weight", p + ".bn2", planes, planes, 3, stride, true, kb);
      blk.conv3 = add_conv(e, p + ".conv3.weight", p + ".bn3", planes, cout, 1, 1, false, kb);
      blk.down = b == 0 ? add_conv(e, p + ".downsample.0.weight", p + ".downsample.1", cin, cout, 1, stride, false, kb) : -1;
      if (li >= 1) {
        TdnMse m;
        m.c = planes;
        m.key = p;
        blk.mse = (int)e->tdn_mse.size();
        e->tdn_mse.push_back(m);
      }
      e->blocks.push_back(blk);
      cin = cout;
    }
  }
  e->feat = 4 * kPlanes[3];
}

void build_resnet_topology(tsm_engine *e) {
  e->convs.clear();
  e->blocks.clear();
  add_conv(e, "base_model.conv1.weight", "base_model.bn1", 3, 64, 7, 2, false);
  const Backbone &bb = *find_backbone(e->depth);
  const int expansion = bb.basic ? 1 : 4;
  int cin = 64;
  for (int li = 0; li < 4; ++li) {
    for (int b = 0; b < bb.blocks[li]; ++b) {
      const int planes = kPlanes[li], cout = planes * expansion;
      const int mid = planes * e->width / 64;   // (Bottleneck only: a BasicBlock engine is always width 64)
      const int stride = (b == 0 && li > 0) ? 2 : 1;
      // block placement wraps the whole block in TemporalShift: its tensors are "layerL.B.net.<name>", conv1 unwrapped
      const bool bp = e->place == 1;
      // a non-local engine wraps some blocks once more: their own tensors move under "layerL.B.block", the new ones are "layerL.B.nl.*"
      const bool nl = e->non_local && !bb.basic && nonlocal_wrapped(li + 1, b);
      const std::string lb = "base_model.layer" + std::to_string(li + 1) + "." + std::to_string(b);
      const std::string p = lb + (nl ? ".block" : "") + (bp ? ".net" : "");
      const std::string c1key = p + (bp ? ".conv1.weight" : ".conv1.net.weight");
      Block blk;
      blk.stride = stride;
      blk.T = e->temporal_pool && li > 0 ? temporal_pool_segments(e->cfg.num_segments) : e->cfg.num_segments;
      blk.tpool_after = e->temporal_pool && li == 0 && b == bb.blocks[0] - 1;
      blk.name = "layer" + std::to_string(li + 1) + "." + std::to_string(b);
      if (bb.basic) {
        // conv1: 3x3 at the block's stride, the temporal shift fused into its loader (which has no segmented form);
        // conv2: 3x3, + identity.  Downsample (1x1 at the stride) where the width or the size changes.
        blk.conv1 = add_conv(e, c1key, p + ".bn1", cin, planes, 3, stride, !e->cfg.is_shift);
        blk.conv2 = add_conv(e, p + ".conv2.weight", p + ".bn2", planes, planes, 3, 1, false);
        blk.conv3 = -1;
      } else {   // conv1 1x1 (shifted), conv2 3x3 at the stride, conv3 1x1 + identity; downsample in every stage's first block
        blk.conv1 = add_conv(e, c1key, p + ".bn1", cin, mid, 1, 1, true);
        blk.conv2 = add_conv(e, p + ".conv2.weight", p + ".bn2", mid, mid, 3, stride, true);
        blk.conv3 = add_conv(e, p + ".conv3.weight", p + ".bn3", mid, cout, 1, 1, false);
      }
      const bool down = bb.basic ? (stride != 1 || cin != planes) : b == 0;
      blk.down = down ? add_conv(e, p + ".downsample.0.weight", p + ".downsample.1", cin, cout, 1, stride, false) : -1;
      blk.out_name = blk.name + (nl ? ".block" : "");
      if (nl) {   // theta | phi | g: cout -> 3 * cout / 2 (bias, no BN, no ReLU); W: cout / 2 -> cout (bias + BN, + x, no ReLU)
        blk.nl_qkv = add_conv(e, lb + ".nl.theta.weight", "", cout, 3 * (cout / 2), 1, 1, false, ConvKind::kNlQkv);
        blk.nl_w = add_conv(e, lb + ".nl.W.0.weight", lb + ".nl.W.1", cout / 2, cout, 1, 1, false, ConvKind::kNlW);
        e->convs[blk.nl_qkv].nlp = e->convs[blk.nl_w].nlp = lb + ".nl";
      }
      e->blocks.push_back(blk);
      cin = cout;
    }
  }
  e->feat = kPlanes[3] * expansion;
}

// The spelling of an engine key without the non-local wrapper's ".block" ("" when it has none).
std::string without_block(const std::string &key) {
  const size_t at = key.find(".block.");
  return at == std::string::npos ? "" : key.substr(0, at) + key.substr(at + 6);
}

// The un-wrapped spelling of an engine key, also accepted: TemporalShift wraps conv1 as ".conv1.net.weight" (blockres) or the
// whole block as "layerL.B.net.<name>" (block placement); "" when the key has no wrapper.
std::string unwrapped(const tsm_engine *e, const std::string &key) {
  if (e->place == 1) {
    const size_t at = key.find(".net.");
    return at == std::string::npos ? "" : key.substr(0, at) + key.substr(at + 4);
  }
  const std::string net = ".conv1.net.weight";
  if (key.size() > net.size() && key.compare(key.size() - net.size(), net.size(), net) == 0)
    return key.substr(0, key.size() - net.size()) + ".conv1.weight";
  return "";
}

// A temporal-pool engine: the spelling of a layer2 key under the TemporalPool wrapper, which holds the stage as `net`
// ("base_model.layer2.net.<b>.<rest>"); "" for any other key or engine.
std::string pool_wrapped(const tsm_engine *e, const std::string &key) {
  const std::string stage = "base_model.layer2.";
  return e->temporal_pool && key.compare(0, stage.size(), stage) == 0 ? stage + "net." + key.substr(stage.size()) : "";
}

// f(spelling) for an engine key and every other spelling of it a checkpoint may use -- without the shift wrapper, without the
// non-local wrapper, without both; the key and its unwrapped form under the temporal pool's wrapper -- in this order, until one
// call returns true.
template <class F>
bool spellings(const tsm_engine *e, const std::string &key, F f) {
  if (f(key)) return true;
  const std::string uw = unwrapped(e, key), nb = without_block(key), both = nb.empty() ? nb : unwrapped(e, nb);
  const std::string pooled = pool_wrapped(e, key), pooled_uw = pool_wrapped(e, uw);
  for (const std::string *alt : {&uw, &nb, &both, &pooled, &pooled_uw})
    if (!alt->empty() && f(*alt)) return true;
  return false;
}

const HostTensor *find_tensor(const tsm_engine *e, const std::string &key) {
  const HostTensor *hit = nullptr;
  spellings(e, key, [&](const std::string &s) {
    const auto it = e->tensors.find(s);
    if (it != e->tensors.end()) hit = &it->second;
    return hit != nullptr;
  });
  return hit;
}

// The values of a manifest tensor, behind tsm_finalize's check_tensors: it is there, in its shape.
const std::vector<float> &tensor(const tsm_engine *e, const std::string &key) { return find_tensor(e, key)->data; }

// What tsm_set_tensor accepts: a manifest key in any of its spellings.
bool known_name(const tsm_engine *e, const std::string &name) {
  for (const TensorSpec &t : e->manifest)
    if (spellings(e, t.key, [&](const std::string &s) { return s == name; })) return true;
  return false;
}

// Key suffixes that more than one place needs.  A BatchNorm `bnp`: its four vectors, then the counter checkpoints carry.
const char *const kBnSuffix[] = {".weight", ".bias", ".running_mean", ".running_var", ".num_batches_tracked"};
// A non-local block `nlp`: the three convs that make the theta | phi | g conv, in its row order.
const char *const kNlQkv[3] = {".theta", ".phi.0", ".g.0"};
// A TDN long-term module `key`: its five convs and the temporal conv, then its BatchNorms (tdn_pack_mse's argument order).
enum { kMseConv1, kMseConv2, kMseConv3, kMseSmall2, kMseSmall4, kMseTemporal, kMseConvs };
const char *const kTdnMseConvs[kMseConvs] = {".mse.conv1.weight", ".mse.conv2.weight", ".mse.conv3.weight", ".mse.conv3_smallscale2.weight",
                                             ".mse.conv3_smallscale4.weight", ".shift.conv.weight"};
enum { kMseBn1, kMseBnSmall2, kMseBnSmall4, kMseBn3, kMseBns };
const char *const kTdnMseBns[kMseBns] = {".mse.bn1", ".mse.bn3_smallscale2", ".mse.bn3_smallscale4", ".mse.bn3"};

std::string bias_key(const std::string &wkey) { return wkey.substr(0, wkey.size() - 6) + "bias"; }   // "<name>.bias" of "<name>.weight"
const char *head_prefix(const tsm_engine *e) { return e->convnext ? "head.fc" : e->tdn ? "new_fc" : "fc"; }   // the classifier

// The engine's tensor manifest, from its topology: per conv by kind, then the family's other tensors, then the classifier --
// the order in which tsm_finalize reports a defect.  The refusal texts are formed here because they differ by group: a ResNet's
// BatchNorm and classifier are named as a whole, everything else by its own key.
void build_manifest(tsm_engine *e) {
  using Shape = std::vector<int64_t>;
  std::vector<TensorSpec> &m = e->manifest;
  m.clear();
  auto want = [&](const std::string &key, Shape shape, bool joins = false) {
    m.push_back({key, std::move(shape), "missing " + key, "shape mismatch for " + key, joins, false});
  };
  auto want_pair = [&](const std::string &wkey, Shape shape, bool joins = false) {   // "<name>.weight" and "<name>.bias" [shape[0]]
    want(wkey, shape);
    want(bias_key(wkey), {shape[0]}, joins);
  };
  auto ignore = [&](const std::string &key) { m.push_back({key, {}, "", "", false, true}); };
  auto want_bn = [&](const std::string &bnp, int c, bool joins, bool as_a_whole) {
    for (int i = 0; i < 4; ++i) {
      want(bnp + kBnSuffix[i], {c}, joins);
      if (as_a_whole) {
        m.back().missing = "missing BatchNorm tensors of " + bnp;
        m.back().mismatch = "BN shape mismatch for " + bnp;
      }
    }
    ignore(bnp + kBnSuffix[4]);
  };
  for (const ConvLayer &c : e->convs) {
    switch (c.kind) {
      case ConvKind::kBn:   // (the weight's absence, the BatchNorm's absence, then the shapes)
        want(c.wkey, {c.cout, c.cin, c.k, c.k});
        want_bn(c.bnp, c.cout, true, true);
        break;
      case ConvKind::kNlQkv:
        for (const char *part : kNlQkv) want_pair(c.nlp + part + ".weight", {c.cout / 3, c.cin, 1, 1, 1}, true);
        break;
      case ConvKind::kNlW:
        want_bn(c.bnp, c.cout, false, true);
        want_pair(c.wkey, {c.cout, c.cin, 1, 1, 1}, true);
        break;
      case ConvKind::kCnxStem: want_pair(c.wkey, {c.cout, 3, 4, 4}); break;
      case ConvKind::kCnxDown: want_pair(c.wkey, {c.cout, c.cin / 4, 2, 2}); break;
      case ConvKind::kCnxFc1: want_pair(c.wkey, {c.cout, c.cin}); break;
      case ConvKind::kCnxFc2:
        want_pair(c.wkey, {c.cout, c.cin});
        want(c.gkey, {c.cout});
        break;
      case ConvKind::kTdnBias:
        want(c.wkey, {c.cout, c.cin, c.k, c.k});
        want_bn(c.bnp, c.cout, false, false);
        want(bias_key(c.wkey), {c.cout});
        break;
      case ConvKind::kTdnConv15:
        want(c.wkey, {c.cout, kTdnDiffC, 7, 7});
        want_bn(c.bnp, c.cout, false, false);
        break;
    }
  }
  if (e->convnext) {
    auto want_norm = [&](const CnxNorm &n) { want_pair(n.key + ".weight", {n.c}); };
    want_norm(e->cnx_stem_norm);
    want_norm(e->cnx_head_norm);
    for (const CnxStage &st : e->cnx_stages)
      if (st.down >= 0) want_norm(st.norm);
    for (const CnxBlock &blk : e->cnx_blocks) {
      want_pair(blk.dwkey + ".weight", {blk.c, 1, 7, 7});
      want_norm(blk.norm);
    }
  }
  for (const TdnMse &mse : e->tdn_mse) {
    const int C = mse.c, r = C / kTdnReduction;
    const Shape conv_shapes[kMseConvs] = {{r, C, 1, 1}, {r, 1, 3, 3}, {C, r, 1, 1}, {r, r, 3, 3}, {r, r, 3, 3}, {C, 1, 3}};
    for (int i = 0; i < kMseConvs; ++i) want(mse.key + kTdnMseConvs[i], conv_shapes[i]);
    for (int i = 0; i < kMseBns; ++i) want_bn(mse.key + kTdnMseBns[i], i == kMseBn3 ? C : r, false, false);
  }
  if (e->tdn)   // (in every TDN checkpoint, unused by the forward)
    for (const char *s : {".weight", ".bias"}) ignore(std::string("base_model.conv1_temp") + s);
  const std::string fc = head_prefix(e);
  want_pair(fc + ".weight", {e->cfg.num_class, e->feat}, !e->convnext && !e->tdn);
  if (!e->convnext && !e->tdn)   // (a ResNet's classifier is refused as a pair)
    for (size_t i = m.size() - 2; i < m.size(); ++i) {
      m[i].missing = "missing fc.weight / fc.bias";
      m[i].mismatch = "fc shape mismatch (want [num_class, " + std::to_string(e->feat) + "])";
    }
}

void build_topology(tsm_engine *e) {
  if (e->convnext) build_convnext_topology(e);
  else if (e->tdn) build_tdn_topology(e);
  else build_resnet_topology(e);
  build_manifest(e);
}

// tsm_finalize's check of the host tensors against the manifest, in its order; within a group every absence before any shape.
int check_tensors(tsm_engine *e) {
  const std::vector<TensorSpec> &m = e->manifest;
  for (size_t first = 0, end; first < m.size(); first = end) {
    for (end = first + 1; end < m.size() && m[end].joins;) ++end;
    if (m[first].ignored) continue;
    for (size_t i = first; i < end; ++i)
      if (!find_tensor(e, m[i].key)) return fail(e, TSM_ERR_MISSING_TENSOR, m[i].missing);
    for (size_t i = first; i < end; ++i)
      if (find_tensor(e, m[i].key)->shape != m[i].shape) return fail(e, TSM_ERR_SHAPE, m[i].mismatch);
  }
  return TSM_OK;
}

int dev_alloc(tsm_engine *e, float **p, size_t elems, const char *name = "weights", size_t frame_elems = 0) {
  if (e->poison) {   // between poisoned bands of one frame of this buffer, poison all over until something is written
    GuardBuf g;
    TSM_HIP(e, guard_alloc(&g, name, elems * sizeof(float), frame_elems * sizeof(float)));
    e->allocs.push_back(g.base);
    e->guards.push_back(g);
    *p = g.ptr();
    return TSM_OK;
  }
  void *q = nullptr;
  TSM_HIP(e, hipMalloc(&q, elems * sizeof(float)));
  e->allocs.push_back(q);
  *p = static_cast<float *>(q);
  return TSM_OK;
}

// One weight preparation, for tsm_finalize and tsm_conv_op alike.  Raw OIHW weights + the four BatchNorm vectors of layer c -> the folded fp32 matrix [cout][kp] in c's geometry, and the bias.
void prepare_weights(const ConvLayer &c, const float *w, const float *gamma, const float *beta, const float *mean, const float *var,
                     std::vector<float> *wp, std::vector<float> *bias) {
  if (c.stem_pairs) fold_and_pack_stem_pairs(w, gamma, beta, mean, var, c.cout, c.kp, wp, bias);
  else fold_and_pack(w, gamma, beta, mean, var, c.cout, c.cin, c.k, c.cp, c.kp, wp, bias);
}

// Allocate, then copy.  `alloc(&ptr, name, elems, frame_elems)` returns a status: the engine's dev_alloc, or tsm_conv_op's
// guarded temporaries (e = NULL).
template <class Alloc>
int upload(tsm_engine *e, Alloc &alloc, float **p, const char *name, const std::vector<float> &v, size_t frame_elems = 0) {
  const int rc = alloc(p, name, v.size(), frame_elems);
  if (rc) return rc;
  TSM_HIP(e, hipMemcpy(*p, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
  return TSM_OK;
}

// A folded fp32 matrix [cout][K] (converted in place to the storage format of `prec`) and its bias, to the device.
template <class Alloc>
int upload_conv(tsm_engine *e, Alloc &alloc, int prec, int cout, std::vector<float> *wp, const std::vector<float> &bias, float **d_w,
                float **d_b) {
  to_storage(wp, prec);
  const int rc = upload(e, alloc, d_w, "d_w", *wp, wp->size() / cout);
  return rc ? rc : upload(e, alloc, d_b, "d_b", bias);
}

// TSM_POISON=1, immediately before the first launch of a forward proper: every activation / scratch buffer filled with the
// poison word, so whatever a kernel relies on in them must be written by THIS forward, not inherited.  Weights are not touched.
int poison_workspace(tsm_engine *e, hipStream_t s) {
  if (!e->poison) return TSM_OK;
  const float *targets[] = {e->buf[0], e->buf[1], e->buf[2], e->buf[3], e->buf[4], e->d_in4, e->d_pooled, e->d_logits, e->d_partial, e->d_tap,
                            e->d_patches, e->d_mse[0], e->d_mse[1], e->d_mse[2], e->d_mse[3], e->d_mse[4], e->d_mse[5], e->d_mse[6], e->d_mse[7],
                            e->d_mse[8]};
  for (const GuardBuf &g : e->guards)
    for (const float *t : targets)
      if (t && t == g.ptr())
        TSM_HIP(e, hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(g.ptr()), (int)kPoisonWord, g.lay.payload / 4, s));
  return TSM_OK;
}

// TSM_POISON=1, after a forward's last launch: synchronise and verify the bands of every buffer.
int verify_guards(tsm_engine *e, hipStream_t s) {
  if (!e->poison) return TSM_OK;
  TSM_HIP(e, hipStreamSynchronize(s));
  for (const GuardBuf &g : e->guards) {
    std::string msg;
    TSM_HIP(e, guard_verify(g, &msg));
    if (!msg.empty()) return fail(e, TSM_ERR_GUARD, msg);
  }
  return TSM_OK;
}

// (the shapes: tsm_host_util.h, conv_shape_params / second_source_shape)
tsm::ConvParams make_params(const ConvLayer &c, const float *x, const float *res, float *y, int n, int hi,
                            int wi, bool relu, int T, int shift_div, int prec = tsm::kPrecF32) {
  tsm::ConvParams p = conv_shape_params(c, c.k, c.stride, c.cout, n, hi, wi, relu, T, shift_div, prec, res != nullptr);
  p.x = x; p.w = c.d_w; p.bias = c.d_b; p.res = res; p.y = y;
  return p;
}

// A second source behind p's own K: one GEMM over K = [p's K | kp2] (Bottleneck.conv3 + the downsample branch, concat_k_pair's
// matrix; the caller sets p->w and p->bias).  x2 is [N, hi2, wi2, c2], read at stride2.
void set_second_source(tsm::ConvParams *p, int kp2, const float *x2, int c2, int hi2, int wi2, int stride2) {
  second_source_shape(p, kp2, c2, hi2, wi2, stride2);
  p->x2 = x2;
}

// $XDG_CACHE_HOME/tsm_hip/tune_cache.txt, else $HOME/.cache/tsm_hip/tune_cache.txt ("" when neither is set or the
// directory cannot be made: no cache, never an error).
std::string default_tune_cache_path() {
  std::string base;
  if (const char *x = getenv("XDG_CACHE_HOME")) base = x;
  if (base.empty()) {
    const char *h = getenv("HOME");
    if (!h || !*h) return "";
    base = std::string(h) + "/.cache";
    (void)mkdir(base.c_str(), 0700);
  }
  base += "/tsm_hip";
  if (mkdir(base.c_str(), 0700) != 0 && errno != EEXIST) return "";
  return base + "/tune_cache.txt";
}

bool tune_cache_load(tsm_engine *e, int key, std::vector<int> *codes) {
  if (e->tune_path.empty()) return false;
  FILE *f = fopen(e->tune_path.c_str(), "r");
  if (!f) return false;
  const std::string want = e->tune_sig + "|" + std::to_string(key) + "|";
  char line[4096];
  bool ok = false;
  while (!ok && fgets(line, sizeof line, f)) ok = parse_tune_line(line, want, tsm::kNumTiles, codes);
  fclose(f);
  return ok;
}

void tune_cache_store(tsm_engine *e, int key, const std::vector<int> &codes) {
  if (e->tune_path.empty()) return;
  std::string line = e->tune_sig + "|" + std::to_string(key) + "|";
  for (size_t i = 0; i < codes.size(); ++i) line += (i ? "," : "") + std::to_string(codes[i]);
  line += "\n";
  if (line.size() >= 4096) return;
  FILE *f = fopen(e->tune_path.c_str(), "a");   // one short write per line: appends from several ranks do not interleave
  if (!f) return;
  fwrite(line.data(), 1, line.size(), f);
  fclose(f);
}

// The tail split of a segmented 64x64 launch (tile code bit kCodeTailK): tsm_host_util.h::tail_split_point on this launch's shape.
bool tail_split_from(const tsm::ConvParams &p, int n_cu, size_t partial_elems, int *tail_from) {
  if (p.kseg_len <= 0) return false;
  const long from = tsm_host::tail_split_point(p.M, p.Cout, tsm::conv_num_segments(p), n_cu, partial_elems);
  *tail_from = (int)from;
  return from > 0;
}

// A tile code is a ConvTile, plus kCodeSplitK for the split-K form of a segmented layer: one workgroup per (tile, K segment)
// writes raw segment sums, splitk_reduce adds them in segment order and applies bias / ReLU -- bit-identical to the unsplit
// launch.  Every output element accumulates its K in the same order whatever the tiling, so codes are bit-neutral.
// `partial` holds `partial_elems` floats of segment sums (the engine's split-K scratch; the per-op entry point's own).
// `pos_balance`: position-major launches run live-balanced XCD runs (tsm_conv_rules.h::pos_balanced_runs; the same bits either way).
hipError_t launch_conv_code(tsm::ConvParams p, int ks, int code, float *partial, size_t partial_elems, int n_cu, hipStream_t s,
                            bool pos_balance = true) {
  p.tile = code & kCodeTileMask;
  // kCodePosMajor: position-major rows, honoured only where pos_major_valid holds for THIS launch (whole-K or with the tail
  // split; never with kCodeSplitK); anywhere else the bit is ignored and the natural order runs (same bits).
  const bool pos_major = (code & kCodePosMajor) && !(code & kCodeSplitK) && (code & kCodeTileMask) == tsm::kTile64x64 &&
                         tsm::pos_major_valid(p, ks);
  p.pos_major = pos_major ? 1 : 0;
  p.pos_balance = pos_major && pos_balance ? 1 : 0;
  // A cached code may come from a smaller batch of the same bucket: the scratch-size condition is re-checked on
  // EVERY launch (falling back to the whole-K form, which gives the same bits).
  if ((code & kCodeSplitK) && p.kseg_len > 0 &&
      (size_t)tsm::conv_num_segments(p) * (size_t)p.M * (size_t)p.Cout <= partial_elems) {
    float *y = p.y;
    p.ksplit = 1;
    p.y = partial;
    hipError_t st = tsm::launch_conv(p, ks, s);
    if (st == hipSuccess)
      st = tsm::launch_splitk_reduce(partial, tsm::conv_num_segments(p), p.M, p.Cout, p.bias, nullptr, y, p.relu, s);
    return st;
  }
  // kCodeTailK: the tail split (ConvParams::ksplit = 2) of a segmented 64x64 layer -- the tiles of the last, partly filled round
  // of resident workgroups (five per CU) as (tile, segment) pieces.  Re-derived from THIS launch's tile count on every launch;
  // whenever it does not apply the whole-K form runs (same bits).
  if ((code & kCodeTailK) && (code & kCodeTileMask) == tsm::kTile64x64 && p.kseg_len > 0) {
    int tail_from = 0;
    if (tail_split_from(p, n_cu, partial_elems, &tail_from)) {
      float *y = p.y;
      const int mt0 = tail_from / (p.Cout / 64) * 64;
      p.ksplit = 2;
      p.tail_from = tail_from;
      p.ypart = partial;
      hipError_t st = tsm::launch_conv(p, ks, s);
      if (st == hipSuccess && pos_major)   // (the tail's rows are GEMM rows mt0 .. M - 1: the last positions of every frame)
        st = tsm::launch_splitk_reduce_pos(partial, tsm::conv_num_segments(p), mt0, p.M - mt0, p.N, p.Ho * p.Wo, p.Cout, p.bias, y,
                                           p.relu, s);
      else if (st == hipSuccess)
        st = tsm::launch_splitk_reduce(partial, tsm::conv_num_segments(p), p.M - mt0, p.Cout, p.bias, nullptr,
                                       y + (size_t)mt0 * p.Cout, p.relu, s);
      return st;
    }
  }
  return tsm::launch_conv(p, ks, s);
}

// A tile code trusted only after it has been checked against THIS launch: anything else is 0, the heuristic shape (launch_conv_code
// ignores the split bits where they do not apply).
int checked_code(const tsm::ConvParams &p, int code, int n_cu) {
  return code > 0 && (code & ~kCodeValid) == 0 && tsm::conv_tile_valid(p, code & kCodeTileMask, n_cu) ? code : 0;
}

struct Tap {
  const float *ptr = nullptr;
  int64_t shape[4] = {0, 0, 0, 0};
  bool hit = false;
};

// One event before and one after a launch when per-launch timing is armed for this forward.
struct LaunchTimer {
  tsm_engine *e;
  hipStream_t s;
  bool on;
  bool skip;  // armed, but this launch is outside the selection: keep the slot, record nothing
  LaunchTimer(tsm_engine *e_, hipStream_t s_, bool is3x3)
      : e(e_), s(s_), on(e_->cur_timing != nullptr), skip(e_->timing_only3x3 && !is3x3) { mark(); }
  ~LaunchTimer() { mark(); }
  void mark() {
    if (!on) return;
    if (skip) {
      e->cur_timing->push_back(nullptr);
      return;
    }
    hipEvent_t ev = nullptr;
    if (!e->event_pool.empty()) {
      ev = e->event_pool.back();
      e->event_pool.pop_back();
    } else if (hipEventCreate(&ev) != hipSuccess) {
      return;
    }
    (void)hipEventRecord(ev, s);
    e->cur_timing->push_back(ev);
  }
};
#define TSM_LAUNCH_K(e, s, is3x3, call) \
  do {                                  \
    LaunchTimer _lt((e), (s), (is3x3)); \
    TSM_HIP((e), (call));               \
  } while (0)
#define TSM_LAUNCH(e, s, call) TSM_LAUNCH_K(e, s, false, call)

// Keeps `n` launch slots of the per-launch timing (tsm_layer_times) for launches this forward does not make: each is reported
// as "not recorded", so the slots stay those of TsmEngine.launch_names().
void skip_slots(tsm_engine *e, int n) {
  if (e->cur_timing) e->cur_timing->insert(e->cur_timing->end(), 2 * (size_t)n, nullptr);
}

// Times `launches` (enqueues one or more launches on `s`, returns the first error) the way the tuner makes every choice: four
// repetitions, each inside one event bracket (so the boundaries between back-to-back kernels and each kernel's cold start on
// its producer's output are priced, as in a forward), the first discarded (it warms the caches), the best of the other three.
template <class F>
int time_best_of(tsm_engine *e, hipStream_t s, F &&launches, float *best_ms) {
  float ms[4];
  for (int rep = 0; rep < 4; ++rep) {
    TSM_HIP(e, hipEventRecord(e->ev0, s));
    TSM_HIP(e, launches());
    TSM_HIP(e, hipEventRecord(e->ev1, s));
    TSM_HIP(e, hipEventSynchronize(e->ev1));
    TSM_HIP(e, hipEventElapsedTime(&ms[rep], e->ev0, e->ev1));
  }
  *best_ms = std::min(ms[1], std::min(ms[2], ms[3]));
  return TSM_OK;
}

// Segments per clip behind the backbone (the head's, the feature rows', the per-segment logits'): T, or T / 2 behind the temporal pool.
int out_segments(const tsm_engine *e) { return e->temporal_pool ? temporal_pool_segments(e->cfg.num_segments) : e->cfg.num_segments; }

// Block placement with the shift on: every block reads its input through the shift, the identity path included.
bool block_shift(const tsm_engine *e) { return e->place == 1 && e->cfg.is_shift; }

// Every launch Bottleneck k can make on nn frames of hh x ww pixels, x -> y through the branch temporaries t1, t2, with
// `reverse` still 0: the three convs (conv3 with the downsample branch K-concatenated behind it where the block has one) and
// the fused forms.  Built with null tensors too, for the kernels' validity tests, which read shapes only.
struct BlockLaunches {
  tsm::ConvParams p1, p2, p3;
  tsm::BneckParams pb{};     // the whole block (bneck_ws_kernel)
  tsm::FrontParams pfr{};    // shift + conv1 + the stride-2 conv2 (front_s2_kernel; t1 never exists in memory)
  tsm::Fused23Params pf{};   // conv2 + conv3 + residual (tsm::launch_conv23_fused)
  tsm::Conv31Params q{};     // conv3 + residual and the NEXT block's shift + conv1 (conv31_fused_kernel), writing t1
};

BlockLaunches block_launches(const tsm_engine *e, size_t k, int nn, const float *x, float *y, float *t1, float *t2, int hh, int ww) {
  const tsm_config &cfg = e->cfg;
  const Block &blk = e->blocks[k];
  const ConvLayer &c1 = e->convs[blk.conv1], &c2 = e->convs[blk.conv2], &c3 = e->convs[blk.conv3];
  const int T = blk.T, shiftT = cfg.is_shift ? T : 0, prec = e->prec;
  const int ho = conv_out_size(hh, 3, blk.stride), wo = conv_out_size(ww, 3, blk.stride);
  const bool fused = blk.down >= 0;   // (a Bottleneck's downsample always runs inside conv3's GEMM)
  BlockLaunches L;
  L.p1 = make_params(c1, x, nullptr, t1, nn, hh, ww, true, shiftT, cfg.shift_div, prec);
  L.p2 = make_params(c2, t1, nullptr, t2, nn, hh, ww, true, 0, 1, prec);
  L.p3 = make_params(c3, t2, fused ? nullptr : x, y, nn, ho, wo, true, 0, 1, prec);
  if (fused) {
    const ConvLayer &cd = e->convs[blk.down];
    L.p3.w = blk.d_wf; L.p3.bias = blk.d_bf;
    set_second_source(&L.p3, cd.kp, x, cd.cp, hh, ww, blk.stride);
  }
  if (block_shift(e)) {   // block placement: the identity / the downsample operand is the block input through the shift
    L.p3.T = T;
    L.p3.fold = (fused ? e->convs[blk.down].cp : c3.cout) / cfg.shift_div;
  }
  tsm::BneckParams &pb = L.pb;
  pb.x = x; pb.w1 = c1.d_w; pb.bias1 = c1.d_b; pb.w2 = c2.d_w; pb.bias2 = c2.d_b; pb.y = y;
  pb.w3 = fused ? blk.d_wf : c3.d_w; pb.bias3 = fused ? blk.d_bf : c3.d_b;
  pb.cin = c1.cin; pb.N = nn; pb.H = hh; pb.W = ww; pb.T = shiftT; pb.fold = L.p1.fold;
  tsm::FrontParams &pfr = L.pfr;
  pfr.x = x; pfr.w1 = c1.d_w; pfr.bias1 = c1.d_b; pfr.w2 = c2.d_w; pfr.bias2 = c2.d_b; pfr.y = t2;
  pfr.N = nn; pfr.H = hh; pfr.W = ww; pfr.T = shiftT; pfr.fold = L.p1.fold;
  // (conv3's weights in fragment order for fp32 / split-bf16; the bf16 form reads conv3's packed matrix itself)
  tsm::Fused23Params &pf = L.pf;
  pf.x = t1; pf.w2 = c2.d_w; pf.bias2 = c2.d_b; pf.w3f = blk.d_w3f ? blk.d_w3f : c3.d_w; pf.bias3 = c3.d_b; pf.res = x; pf.y = y;
  pf.N = nn; pf.H = hh; pf.W = ww; pf.M = nn * hh * ww; pf.kseg_len = c2.kseg;
  if (k + 1 < e->blocks.size() && e->blocks[k + 1].conv3 >= 0) {
    const ConvLayer &c1n = e->convs[e->blocks[k + 1].conv1];
    tsm::Conv31Params &q = L.q;
    q.t2 = L.p3.x; q.w3 = L.p3.w; q.bias3 = L.p3.bias; q.res = L.p3.res; q.y = L.p3.y;
    q.w1 = c1n.d_w; q.bias1 = c1n.d_b; q.t1 = t1;
    q.n_clips = nn / T; q.T = T; q.HW = ho * wo; q.K3 = L.p3.C; q.C = L.p3.Cout; q.N1 = c1n.cout;
    q.fold = shiftT > 0 ? c1n.cp / cfg.shift_div : 0;
  }
  return L;
}

// The fused forms Bottleneck k of an nn-frame forward on hh x ww inputs CAN run (BasicBlocks have none): dtype, shape, the
// kernels' validity tests, TSM_FUSE_* = 0, and the stage being tapped (a tapped tensor must exist in memory).  `front` does
// not know whether conv1 has already run (BlockPlan::conv1_done).
struct BlockForms {
  bool block = false, front = false, conv23 = false, conv31 = false;
};

BlockForms fused_forms(const tsm_engine *e, size_t k, int nn, int hh, int ww, const char *stage) {
  BlockForms f;
  const Block &blk = e->blocks[k];
  if (blk.conv3 < 0 || block_shift(e)) return f;   // (none of them reads a shifted identity: block placement runs none)
  const ConvLayer &c1 = e->convs[blk.conv1], &c2 = e->convs[blk.conv2], &c3 = e->convs[blk.conv3];
  const BlockLaunches L = block_launches(e, k, nn, nullptr, nullptr, nullptr, nullptr, hh, ww);
  const bool bf16 = e->prec == tsm::kPrecBf16;
  auto want = [&](const char *part) { return stage && blk.name + part == stage; };
  f.block = bf16 && blk.stride == 1 && c1.cout == 64 && c2.cin == 64 && c2.cout == 64 && c3.cout == 256 &&
            (blk.down < 0 ? c1.cin == 256 : c1.cin == 64 && e->convs[blk.down].cp == 64) && e->fuse_block != 0 &&
            tsm::bneck_ws_valid(L.pb.cin, L.pb.N, L.pb.H, L.pb.W, L.pb.T, L.pb.fold) && !want(".conv1") && !want(".conv2");
  f.front = bf16 && blk.stride == 2 && c1.cin == 256 && c1.cout == 128 && c2.cin == 128 && c2.cout == 128 && e->fuse_front != 0 &&
            tsm::front_s2_valid(L.pfr.N, L.pfr.H, L.pfr.W, L.pfr.T, L.pfr.fold) && !want(".conv1");
  f.conv23 = (blk.d_w3f != nullptr || (bf16 && blk.cmid == 64 && tsm::conv23_ws_valid(nn, hh, ww))) && e->fuse23 != 0 &&
             !want(".conv2");
  f.conv31 = bf16 && blk.down < 0 && !blk.tpool_after && k + 1 < e->blocks.size() && e->blocks[k + 1].conv3 >= 0 && e->fuse31 != 0 &&
             tsm::conv31_valid(L.q);
  return f;
}

// What each block of an nn-frame forward runs: a fused form runs where it can (fused_forms) and was chosen -- forced through
// TSM_FUSE_* = 1 or its bit in the tuned code.  At most one form per block, in this precedence: the whole block, the front
// (never when conv1 has already run), conv2 + conv3, conv3 + the next block's conv1; the last sets the next block's
// conv1_done.  BasicBlocks run no fused form.
struct BlockPlan {
  bool block = false, front = false, conv1_done = false, conv23 = false, conv31_next = false;
};

std::vector<BlockPlan> plan_forward(const tsm_engine *e, const std::vector<int> *codes, int nn, const char *stage) {
  std::vector<BlockPlan> plan(e->blocks.size());
  int hh = e->hp, ww = e->wp;
  for (size_t k = 0; k < e->blocks.size(); ++k) {
    const Block &blk = e->blocks[k];
    if (e->tdn && (k == 0 || blk.diff_path != e->blocks[k - 1].diff_path)) {   // a TDN engine: the difference path's maps first, then the trunk's
      hh = blk.diff_path ? e->hd : e->hp;
      ww = blk.diff_path ? e->wd : e->wp;
    }
    const BlockForms can = fused_forms(e, k, nn, hh, ww, stage);
    auto chosen = [&](int force, int conv, int bit) { return force == 1 || (codes && ((*codes)[conv] & bit)); };
    BlockPlan &p = plan[k];
    p.conv1_done = k > 0 && plan[k - 1].conv31_next;
    if (can.block && chosen(e->fuse_block, blk.conv1, kCodeBlock)) p.block = true;
    else if (can.front && !p.conv1_done && chosen(e->fuse_front, blk.conv1, kCodeFront)) p.front = true;
    else if (can.conv23 && chosen(e->fuse23, blk.conv2, kCodeConv23)) p.conv23 = true;
    else if (can.conv31 && chosen(e->fuse31, blk.conv3, kCodeConv31)) p.conv31_next = true;
    hh = conv_out_size(hh, 3, blk.stride);
    ww = conv_out_size(ww, 3, blk.stride);
    if (blk.tpool_after) nn /= 2;   // the temporal pool: layers 2-4 run on half the frames
  }
  return plan;
}

// One forward (run_forward): the state its launches share.
struct Forward {
  tsm_engine *e;
  hipStream_t s;
  const char *stage;
  Tap *tap;
  int prec;
  float *t1, *t2, *idb;                // branch temporaries, the BasicBlock's downsample output
  float *obuf = nullptr;               // a TDN engine: the long-term module's output o, conv2's input in a BottleneckShift (run_tdn sets it)
  std::vector<int> *tiles = nullptr;   // tile codes of this bucket (null: heuristic shapes -- TSM_AUTOTUNE=0 or a tap)
  bool tuning = false;                 // the bucket's tuning pass: time the candidates, write the winners into *tiles
  bool tapped = false;
  // Consecutive conv launches walk their output tiles in opposite directions (ConvParams::reverse): a kernel starts with
  // the rows its predecessor wrote last, which are still in the Infinity Cache / L2 (bit-neutral).
  int flip = 0;
  // (tuning) the previous block and its launches, where its conv3 could also run this block's conv1 (timed at this block's head)
  int prev31 = -1;
  BlockLaunches prev;

  Forward(tsm_engine *e_, hipStream_t s_, const char *stage_, Tap *tap_)
      : e(e_), s(s_), stage(stage_), tap(tap_), prec(e_->prec),
        t1(e_->buf[2]), t2(e_->buf[3]), idb(e_->buf[4]) {}

  // TSM_WALK pins every direction (tests: each walk of each kernel at the engine's geometries); the alternation still
  // advances, so unset leaves the schedule exactly as it is
  int dir(int d) const { return e->walk >= 0 ? e->walk : d; }
  int next_dir() { return dir(flip ^= 1); }
  bool want(const std::string &name) const { return stage && name == stage; }
  int hit(const float *p, int64_t a, int64_t b, int64_t c, int64_t d) {
    tap->ptr = p; tap->shape[0] = a; tap->shape[1] = b; tap->shape[2] = c; tap->shape[3] = d; tap->hit = true;
    tapped = true;
    return TSM_OK;
  }
  hipError_t launch_code(tsm::ConvParams p, int ks, int code);
  hipError_t launch_pair(const tsm::ConvParams &a, int ks_a, int code_a, const tsm::ConvParams &b, int ks_b, int code_b) {
    const hipError_t st = launch_code(a, ks_a, code_a);
    return st != hipSuccess ? st : launch_code(b, ks_b, code_b);
  }
  // (tuning) *wins = the fused launch `one` beat the separate launches `many` it replaces, each timed by time_best_of
  template <class A, class B>
  int fused_wins(A &&many, B &&one, bool *wins) {
    float many_ms = 0.f, one_ms = 0.f;
    int rc = time_best_of(e, s, many, &many_ms);
    if (!rc) rc = time_best_of(e, s, one, &one_ms);
    *wins = one_ms < many_ms;
    return rc;
  }
  int conv(int idx, tsm::ConvParams p, int ks, bool is3x3);
  int run_basic(size_t k, int nn, float *x, float *y, int hh, int ww);
  int run_block(size_t k, const BlockPlan &plan, int nn, float *x, float *y, int hh, int ww);
  int run_nonlocal(size_t k, int nn, float *x, float *z, int hh, int ww);
  int run_mse(size_t k, int nn, int hh, int ww);
  int tune_block(size_t k, int nn, float *x, float *y, int hh, int ww);
};

hipError_t Forward::launch_code(tsm::ConvParams p, int ks, int code) {
  return launch_conv_code(p, ks, code, e->d_partial, e->partial_elems, e->n_cu, s, e->pos_balance);
}

// One conv launch.  Steady forward: the layer's tuned code, trusted only after it has been checked against THIS layer --
// anything else falls back to the heuristic shape, so a stale, foreign or hand-edited cache line can only cost speed.
// Tuning pass: every candidate code timed on the real launch, the fastest kept.
int Forward::conv(int idx, tsm::ConvParams p, int ks, bool is3x3) {
  p.reverse = next_dir();
  if (!tuning) {
    int code = tiles ? (*tiles)[idx] : 0;
    if (e->force_tile) code = e->force_tile;
    if (e->force_code >= 0) code = e->force_code;   // (launch_code ignores the split bit where it does not apply)
    TSM_LAUNCH_K(e, s, is3x3, launch_code(p, ks, checked_code(p, code, e->n_cu)));
    return TSM_OK;
  }
  std::vector<int> cands;
  if (p.kseg_len > 0) {
    // segmented layers: 64x64 / 32x32 tiles, whole-K or split-K (when the segment sums fit the scratch buffer and
    // whole-K tiles alone would leave CUs idle or nearly so), and the tail split where it applies
    const size_t need = (size_t)tsm::conv_num_segments(p) * p.M * p.Cout;
    const long tiles64 = (long)((p.M + 63) / 64) * (p.Cout / 64);
    for (int t : {(int)tsm::kTile64x64, (int)tsm::kTile32x32}) {
      cands.push_back(t);
      if (need <= e->partial_elems && tiles64 < 4L * e->n_cu) cands.push_back(t | kCodeSplitK);
    }
    int tail_from = 0;
    const bool tail = tail_split_from(p, e->n_cu, e->partial_elems, &tail_from);
    if (tail) cands.push_back((int)tsm::kTile64x64 | kCodeTailK);
    // position-major rows (3x3 layers of whole 64-frame batches): the padding taps' MFMAs are not issued
    tsm::ConvParams q = p;
    q.tile = tsm::kTile64x64;
    if (e->pos_major && tsm::pos_major_valid(q, ks)) {
      cands.push_back((int)tsm::kTile64x64 | kCodePosMajor);
      if (tail) cands.push_back((int)tsm::kTile64x64 | kCodePosMajor | kCodeTailK);
    }
  } else {
    for (int t = 1; t < tsm::kNumTiles; ++t)
      if (tsm::conv_tile_valid(p, t, e->n_cu) && (t != tsm::kTile64x128 || e->tile_64x128)) cands.push_back(t);
  }
  float best_ms = 0.f;
  int best = 0;
  for (int t : cands) {
    float ms = 0.f;
    const int rc = time_best_of(e, s, [&] { return launch_code(p, ks, t); }, &ms);
    if (rc) return rc;
    if (best == 0 || ms < best_ms) {
      best = t;
      best_ms = ms;
    }
  }
  (*tiles)[idx] = best;
  return TSM_OK;
}

// One BasicBlock on nn frames: x -> y through t1 (and idb for the downsample), three generic launches:
//   [downsample (1x1 at the stride, its own launch),] shift + conv1 (3x3 at the stride, shift fused into its loader,
//   + ReLU), conv2 (3x3 + identity + ReLU).  None of the Bottleneck fusions applies.
int Forward::run_basic(size_t k, int nn, float *x, float *y, int hh, int ww) {
  const Block &blk = e->blocks[k];
  const std::string &name = blk.name;
  const ConvLayer &c1 = e->convs[blk.conv1], &c2 = e->convs[blk.conv2];
  const int T = blk.T, shiftT = e->cfg.is_shift ? T : 0;   // (the stage's segment count)
  const int ho = conv_out_size(hh, 3, blk.stride), wo = conv_out_size(ww, 3, blk.stride);
  const float *identity = x;
  if (blk.down >= 0) {
    tsm::ConvParams pd = make_params(e->convs[blk.down], x, nullptr, idb, nn, hh, ww, false, block_shift(e) ? shiftT : 0,
                                     e->cfg.shift_div, prec);
    int rcd = conv(blk.down, pd, 1, false);
    if (rcd) return rcd;
    identity = idb;
  }
  tsm::ConvParams p1 = make_params(c1, x, nullptr, t1, nn, hh, ww, true, shiftT, e->cfg.shift_div, prec);
  int rc1 = conv(blk.conv1, p1, 3, true);
  if (rc1) return rc1;
  if (want(name + ".conv1")) return hit(t1, nn, ho, wo, c1.cout);
  tsm::ConvParams p2 = make_params(c2, t1, identity, y, nn, ho, wo, true, 0, 1, prec);
  if (block_shift(e) && blk.down < 0) {   // block placement: the identity is the block input through the shift
    p2.T = T;
    p2.fold = c2.cout / e->cfg.shift_div;
  }
  int rc2 = conv(blk.conv2, p2, 3, true);
  if (rc2) return rc2;
  if (want(name)) return hit(y, nn, ho, wo, c2.cout);
  return TSM_OK;
}

// One Bottleneck of a forward on nn frames, x -> y, as `plan` says.  Its timing slots are the downsample's (which always runs
// inside conv3's GEMM), conv1's, conv2's and conv3's; a fused launch takes the slot of the first launch it replaces and leaves
// the others not recorded.
int Forward::run_block(size_t k, const BlockPlan &plan, int nn, float *x, float *y, int hh, int ww) {
  const Block &blk = e->blocks[k];
  const std::string &name = blk.name;
  const int c1out = e->convs[blk.conv1].cout, c2out = e->convs[blk.conv2].cout, c3out = e->convs[blk.conv3].cout;
  const int ho = conv_out_size(hh, 3, blk.stride), wo = conv_out_size(ww, 3, blk.stride);
  BlockLaunches L = block_launches(e, k, nn, x, y, t1, t2, hh, ww);
  if (blk.mse >= 0) L.p2.x = L.pf.x = obuf;   // a BottleneckShift: conv2 reads the long-term module's output, not conv1's
  if (blk.down >= 0) skip_slots(e, 1);
  if (plan.block) {
    L.pb.reverse = next_dir();
    TSM_LAUNCH(e, s, tsm::launch_bneck_ws(L.pb, s));
    skip_slots(e, 2);   // conv2, conv3
    return want(blk.out_name) ? hit(y, nn, ho, wo, c3out) : TSM_OK;
  }
  if (plan.front) {
    L.pfr.reverse = next_dir();
    TSM_LAUNCH(e, s, tsm::launch_front_s2(L.pfr, s));
    next_dir();         // (it stands for two launches: conv3 keeps the direction it would have had)
    skip_slots(e, 1);   // conv2
  } else {
    if (plan.conv1_done) {
      skip_slots(e, 1);   // the previous block's conv3 launch has left this conv1's output in t1
    } else {
      int rc1 = conv(blk.conv1, L.p1, 1, false);
      if (rc1) return rc1;
    }
    if (want(name + ".conv1")) return hit(t1, nn, hh, ww, c1out);
    if (blk.mse >= 0) {
      const int rcm = run_mse(k, nn, hh, ww);
      if (rcm || tapped) return rcm;
    }
    if (plan.conv23) {
      L.pf.reverse = next_dir();
      TSM_LAUNCH_K(e, s, true, tsm::launch_conv23_fused(L.pf, blk.cmid, blk.cout3, prec, s));
      skip_slots(e, 1);   // conv3
      return want(blk.out_name) ? hit(y, nn, ho, wo, c3out) : TSM_OK;
    }
    int rc2 = conv(blk.conv2, L.p2, 3, true);
    if (rc2) return rc2;
  }
  if (want(name + ".conv2")) return hit(t2, nn, ho, wo, c2out);
  if (plan.conv31_next) {
    L.q.reverse = next_dir();
    TSM_LAUNCH(e, s, tsm::launch_conv31_fused(L.q, s));
  } else {
    int rc3 = conv(blk.conv3, L.p3, 1, false);
    if (rc3) return rc3;
  }
  return want(blk.out_name) ? hit(y, nn, ho, wo, c3out) : TSM_OK;
}

// The non-local block behind wrapped Bottleneck k (steady forward and tuning pass alike: its two convs go through conv(), the
// pool and the attention have one form each): x = the block's output [nn, hh, ww, C], z = BN(W y + b) + x.  Four launches, four
// timing slots:
//   theta | phi | g as ONE 1x1 conv C -> 3 d into t1 (d = C / 2);
//   the 2x2 max-pool of the phi | g channels [d, 3 d) of t1 into t2, dense [nn, hh / 2, ww / 2, 2 d];
//   the attention per clip, theta read in place (ldq = 3 d), phi = t2's channels [0, d), g = [d, 2 d), y [nn * hh * ww, d] into idb;
//   W as a 1x1 conv d -> C with the residual x.
// t1, t2 and idb are free here: the branch temporaries are dead behind the block, and only BasicBlocks use idb.
int Forward::run_nonlocal(size_t k, int nn, float *x, float *z, int hh, int ww) {
  const Block &blk = e->blocks[k];
  const ConvLayer &cq = e->convs[blk.nl_qkv], &cw = e->convs[blk.nl_w];
  const int d = cw.cin, T = blk.T;
  const int64_t nq = nonlocal_positions(T, hh, ww), nkeys = nonlocal_keys(T, hh, ww);
  if (nq <= 0 || nkeys <= 0) return fail(e, TSM_ERR_UNSUPPORTED, blk.name + ": a non-local block needs at least 2 x 2 pixels");
  int rc = conv(blk.nl_qkv, make_params(cq, x, nullptr, t1, nn, hh, ww, false, 0, 1, prec), 1, false);
  if (rc) return rc;
  TSM_LAUNCH(e, s, tsm::launch_maxpool2x2(t1, 3 * d, d, 2 * d, t2, nn, hh, ww, s));
  TSM_LAUNCH(e, s, tsm::launch_nonlocal_attention(t1, 3 * d, t2, t2 + d, 2 * d, idb, d, nn / T, (int)nq, (int)nkeys, d, s));
  if (want(blk.name + ".nl.y")) return hit(idb, nn, hh, ww, d);
  rc = conv(blk.nl_w, make_params(cw, idb, x, z, nn, hh, ww, false, 0, 1, prec), 1, false);
  if (rc) return rc;
  return want(blk.name) ? hit(z, nn, hh, ww, cw.cout) : TSM_OK;
}

// The long-term module of BottleneckShift k of a TDN engine, between conv1 (its output in t1, nn frames of hh x ww pixels) and
// conv2 (which reads obuf).  Five launches, five timing slots: mse_squeeze (the first of the two readers of t1), mse_diff, mse_s2,
// mse_mix -- all on r = C / 16 channels -- and mse_excite_shift, the second reader of t1 and the only writer of a full-width
// tensor, o.  Taps: ".mse.fwd" / ".mse.bwd" (m+ / m-), ".shift" (o).
int Forward::run_mse(size_t k, int nn, int hh, int ww) {
  const Block &blk = e->blocks[k];
  const TdnMse &m = e->tdn_mse[blk.mse];
  const int c = m.c, r = c / kTdnReduction, T = blk.T, hq = tdn_pool_size(hh), wq = tdn_pool_size(ww);
  float *const *q = e->d_mse;   // b, d+, d-, m+, m-, pooled d+, pooled d-, s2+, s2-
  TSM_LAUNCH(e, s, tsm::launch_mse_squeeze(t1, m.d_wq, m.d_bq, q[0], (int64_t)nn * hh * ww, c, s));
  TSM_LAUNCH(e, s, tsm::launch_mse_diff(q[0], m.d_dw, q[1], q[2], q[5], q[6], nn, T, hh, ww, c, s));
  TSM_LAUNCH(e, s, tsm::launch_mse_s2(q[5], q[6], m.d_k2, m.d_b2, q[7], q[8], nn, hq, wq, c, s));
  TSM_LAUNCH(e, s, tsm::launch_mse_mix(q[1], q[2], q[7], q[8], m.d_k4, m.d_b4, q[3], q[4], nn, hh, ww, c, s));
  if (want(blk.name + ".mse.fwd")) return hit(q[3], nn, hh, ww, r);
  if (want(blk.name + ".mse.bwd")) return hit(q[4], nn, hh, ww, r);
  TSM_LAUNCH(e, s, tsm::launch_mse_excite_shift(t1, q[3], q[4], m.d_w3, m.d_b3, m.d_wt, obuf, nn / T, T, hh * ww, c, s));
  if (want(blk.name + ".shift")) return hit(obuf, nn, hh, ww, c);
  return TSM_OK;
}

// One Bottleneck of the tuning pass: the candidate codes of conv1, conv2 and conv3 (conv()), and each fused form that can run
// and that TSM_FUSE_* leaves to the tuner, timed against the tuned launches it replaces (same bits).  Every arm walks as in a
// forward -- separate launches alternate r1, !r1, r1; a fused launch walks like the first launch it replaces -- so both arms
// see the producer / consumer cache reuse of a real forward.  The conv3 + next conv1 form of the PREVIOUS block is
// timed here, once this conv1 is tuned.
int Forward::tune_block(size_t k, int nn, float *x, float *y, int hh, int ww) {
  const Block &blk = e->blocks[k];
  std::vector<int> &codes = *tiles;
  const BlockForms can = fused_forms(e, k, nn, hh, ww, nullptr);
  BlockLaunches L = block_launches(e, k, nn, x, y, t1, t2, hh, ww);
  if (blk.mse >= 0) L.p2.x = L.pf.x = obuf;   // (as run_block)
  const int r1 = flip ^ 1;   // the walk direction conv() is about to give conv1
  bool wins = false;
  int rc = conv(blk.conv1, L.p1, 1, false);
  if (rc) return rc;
  if (blk.mse >= 0 && (rc = run_mse(k, nn, hh, ww))) return rc;   // (one form, nothing to time: run so that its kernels are loaded)
  L.p1.reverse = dir(r1);
  if (prev31 >= 0 && e->fuse31 < 0) {   // the previous block's conv3 + this conv1 as one launch (both arms write the same bits)
    const int conv3 = e->blocks[prev31].conv3, code3 = codes[conv3], code1 = codes[blk.conv1];
    tsm::ConvParams pc = L.p1;
    pc.reverse = dir(prev.p3.reverse ^ 1);
    prev.q.reverse = prev.p3.reverse;
    rc = fused_wins([&] { return launch_pair(prev.p3, 1, code3, pc, 1, code1); },
                    [&] { return tsm::launch_conv31_fused(prev.q, s); }, &wins);
    if (rc) return rc;
    if (wins) codes[conv3] |= kCodeConv31;
  }
  rc = conv(blk.conv2, L.p2, 3, true);
  if (rc) return rc;
  L.p2.reverse = dir(r1 ^ 1);
  if (can.front && e->fuse_front < 0) {   // shift + conv1 + conv2 as one launch (both arms write the same bits to t2)
    const int code1 = codes[blk.conv1], code2 = codes[blk.conv2];
    L.pfr.reverse = dir(r1);
    rc = fused_wins([&] { return launch_pair(L.p1, 1, code1, L.p2, 3, code2); },
                    [&] { return tsm::launch_front_s2(L.pfr, s); }, &wins);
    if (rc) return rc;
    if (wins) codes[blk.conv1] |= kCodeFront;
  }
  rc = conv(blk.conv3, L.p3, 1, false);
  if (rc) return rc;
  L.p3.reverse = dir(r1);   // (what conv() gave it: r1, !r1, r1)
  prev31 = can.conv31 ? (int)k : -1;
  prev = L;
  const int code1 = codes[blk.conv1], code2 = codes[blk.conv2], code3 = codes[blk.conv3];
  L.pf.reverse = dir(r1 ^ 1);
  L.pb.reverse = dir(r1);
  auto pair = [&] { return launch_pair(L.p2, 3, code2, L.p3, 1, code3); };
  auto fused23 = [&] { return tsm::launch_conv23_fused(L.pf, blk.cmid, blk.cout3, prec, s); };
  bool use_fused = can.conv23 && e->fuse23 == 1;
  if (can.conv23 && e->fuse23 < 0) {   // conv2 + conv3 as one launch against the pair
    rc = fused_wins(pair, fused23, &use_fused);
    if (rc) return rc;
    if (use_fused) codes[blk.conv2] |= kCodeConv23;
  }
  if (can.block && e->fuse_block < 0) {   // the whole block as one launch against conv1 + the better form of the rest
    rc = fused_wins([&] {
      const hipError_t st = launch_code(L.p1, 1, code1);
      return st != hipSuccess ? st : use_fused ? fused23() : pair();
    }, [&] { return tsm::launch_bneck_ws(L.pb, s); }, &wins);
    if (rc) return rc;
    if (wins) codes[blk.conv1] |= kCodeBlock;
  }
  return TSM_OK;
}

// The forward of a ConvNeXt engine (tsm_set_convnext) on n frames, the block schedule beside the ResNet one.  Launches and
// timing slots, in order:
//   pack_input (skipped for a packed input), stem.pack, stem.conv, stem.norm;
//   per stage s > 0: stages.s.downsample.norm (LayerNorm + space-to-depth), stages.s.downsample (the 1x1 GEMM over it);
//   per block: .dwln (depthwise 7x7 + LayerNorm), .fc1, .gelu, .fc2 (+ the block input, gamma folded in);
//   head.pool, head.norm, head (tsm_forward_features: the pool kernel once more over the normalised rows, which copies them or
//   divides them by their norm).
// Buffers: the block input in cur, its output in out; t1 holds the normalised tensor a GEMM reads (and the stem's patches),
// t2 the stem's GEMM output, fc1's output (GELU in place) and the pooled rows.
int run_convnext(tsm_engine *e, Forward &f, const float *d_clips, int layout, int n, float *d_logits, hipStream_t s) {
  const tsm_config &cfg = e->cfg;
  const int prec = e->prec;
  const float *in4 = e->d_in4;
  if (layout >= TSM_LAYOUT_NTHWC4) {
    in4 = d_clips;
    skip_slots(e, 1);
  } else {
    TSM_LAUNCH(e, s, tsm::launch_pack_input(d_clips, e->d_in4, n, cfg.height, cfg.width, layout == TSM_LAYOUT_NTCHW ? 1 : 0, prec, s));
  }
  if (f.want("input")) return f.hit(in4, n, cfg.height, cfg.width, 4);
  float *cur = e->buf[0], *out = e->buf[1], *t1 = f.t1, *t2 = f.t2;
  int h = cnx_stem_size(cfg.height), w = cnx_stem_size(cfg.width);
  TSM_LAUNCH(e, s, tsm::launch_stem_pack4(in4, t1, n, cfg.height, cfg.width, s));
  int rc = f.conv(0, make_params(e->convs[0], t1, nullptr, t2, n, h, w, false, 0, 1, prec), 1, false);
  if (rc) return rc;
  TSM_LAUNCH(e, s, tsm::launch_layer_norm(t2, e->cnx_stem_norm.d_w, e->cnx_stem_norm.d_b, cur, (int64_t)n * h * w, kCnxWidths[0], s));
  if (f.want("stem")) return f.hit(cur, n, h, w, kCnxWidths[0]);
  for (int si = 0; si < kCnxStages; ++si) {
    const CnxStage &st = e->cnx_stages[si];
    const int c = kCnxWidths[si];
    if (st.down >= 0) {
      TSM_LAUNCH(e, s, tsm::launch_layer_norm_s2d(cur, st.norm.d_w, st.norm.d_b, t1, n, h, w, c / 2, s));
      h = cnx_down_size(h);
      w = cnx_down_size(w);
      rc = f.conv(st.down, make_params(e->convs[st.down], t1, nullptr, out, n, h, w, false, 0, 1, prec), 1, false);
      if (rc) return rc;
      std::swap(cur, out);
      if (f.want("stages." + std::to_string(si) + ".downsample")) return f.hit(cur, n, h, w, c);
    }
    for (int b = st.first; b < st.first + st.count; ++b) {
      const CnxBlock &blk = e->cnx_blocks[b];
      TSM_LAUNCH(e, s, tsm::launch_dwconv7_ln(cur, blk.d_dw, blk.d_dwb, blk.norm.d_w, blk.norm.d_b, t1, n, h, w, c, s));
      if (f.want(blk.name + ".dwln")) return f.hit(t1, n, h, w, c);
      rc = f.conv(blk.fc1, make_params(e->convs[blk.fc1], t1, nullptr, t2, n, h, w, false, 0, 1, prec), 1, false);
      if (rc) return rc;
      TSM_LAUNCH(e, s, tsm::launch_gelu(t2, (int64_t)n * h * w * c, s));   // (4 c channels: c quads per pixel)
      if (f.want(blk.name + ".fc1")) return f.hit(t2, n, h, w, 4 * c);
      rc = f.conv(blk.fc2, make_params(e->convs[blk.fc2], t2, cur, out, n, h, w, false, 0, 1, prec), 1, false);
      if (rc) return rc;
      std::swap(cur, out);
      if (f.want(blk.name)) return f.hit(cur, n, h, w, c);
    }
  }
  TSM_LAUNCH(e, s, tsm::launch_pool_features(cur, t2, nullptr, n, h * w, e->feat, prec, s));
  if (f.want("head.pool")) return f.hit(t2, n, 1, 1, e->feat);
  TSM_LAUNCH(e, s, tsm::launch_layer_norm(t2, e->cnx_head_norm.d_w, e->cnx_head_norm.d_b, t1, n, e->feat, s));
  if (f.want("head.norm")) return f.hit(t1, n, 1, 1, e->feat);
  if (f.stage) return fail(e, TSM_ERR_INVALID_ARG, std::string("unknown stage: ") + f.stage);
  if (e->features) {   // tsm_forward_features: the normalised rows, or (normalize) each over its Euclidean norm
    TSM_LAUNCH(e, s, tsm::launch_pool_features(t1, e->features == 1 ? d_logits : nullptr, e->features == 2 ? d_logits : nullptr, n, 1,
                                               e->feat, prec, s));
    return TSM_OK;
  }
  TSM_LAUNCH(e, s, tsm::launch_head(t1, e->d_fcw, e->d_fcb, e->d_pooled, d_logits, n, 1, 1, e->feat, cfg.num_class, prec, s));
  return TSM_OK;
}

// The head of a ResNet-shaped engine over the last block's output `cur` [n, hw, feat] -- one launch, one timing slot: the pooled
// (or unit) rows of tsm_forward_features, the per-segment logits of an identity engine, or pool + fc + the mean over the segments.
int run_head(tsm_engine *e, const float *cur, int n, int n_clips, int hw, float *d_logits, hipStream_t s, const char *stage) {
  const int prec = e->prec;
  if (stage) return fail(e, TSM_ERR_INVALID_ARG, std::string("unknown stage: ") + stage);
  if (e->features) {   // tsm_forward_features: d_logits is the [n, feat] output; the pool launch takes the head's timing slot
    TSM_LAUNCH(e, s, tsm::launch_pool_features(cur, e->features == 1 ? d_logits : nullptr, e->features == 2 ? d_logits : nullptr, n,
                                               hw, e->feat, prec, s));
    return TSM_OK;
  }
  if (e->consensus == 1) {   // per-segment logits: one launch, d_pooled is not written (the head's one timing slot either way)
    TSM_LAUNCH(e, s, tsm::launch_head_segments(cur, e->d_fcw, e->d_fcb, d_logits, n, hw, e->feat, e->cfg.num_class, prec, s));
    return TSM_OK;
  }
  TSM_LAUNCH(e, s, tsm::launch_head(cur, e->d_fcw, e->d_fcb, e->d_pooled, d_logits, n_clips, out_segments(e), hw, e->feat,
                                    e->cfg.num_class, prec, s));
  return TSM_OK;
}

// The forward of a TDN engine (tsm_set_tdn) on n_clips clips of T segments, x [n_clips, T, 15, H, W].  Launches and timing slots,
// in order (TsmEngine.launch_names spells them):
//   per chunk of at most tdn_chunk clips: diff.front (tdn_front_kernel, or for TSM_LAYOUT_TDN_POOL tdn_front_pool_kernel over
//     e->tdn_pool with the table / first clip advanced by the chunk: the centre frames into d_in4, the patch rows of the chunk),
//     diff.conv1_5 (the 1x1 GEMM over them into the chunk's rows of x_c5); a forward of fewer chunks than the engine's
//     capacity holds leaves the other chunks' slots not recorded;
//   diff.maxpool (xd0); conv1 (the fp32 stem with its fused max-pool, from d_in4), fuse1;
//   per block of resnext_layer1: [downsample,] conv1, conv2, conv3 -- as every Bottleneck (run_block);
//   per block of layer1: the same; fuse2;
//   per BottleneckShift of layers 2 - 4: [downsample,] conv1, mse_squeeze, mse_diff, mse_s2, mse_mix, mse_excite_shift, conv2, conv3;
//   head.
// Buffers: xd0 in buf[0] and the stem's output in buf[4]; resnext_layer1 rotates buf[0] and buf[1], the trunk buf[4] and whichever
// of buf[0] / buf[1] does not hold xd1; behind fuse2 xd1's buffer is dead and holds o, the long-term module's output.
//
// The two phases (include/tsm_hip.h, beside tsm_set_tdn) cut this schedule in front of fuse2 and keep its timing slots:
//   TSM_LAYOUT_TDN_SEGMENTS: n_clips counts segments; the launches up to layer1's last block, the last blocks of resnext_layer1 and
//     layer1 writing to e->tdn_seg.out_d / out_a; the slots of fuse2 and everything behind it are skipped;
//   TSM_LAYOUT_TDN_RING: the slots in front of fuse2 are skipped; tdn_fuse_ring_kernel writes x from e->tdn_ring into buf[4] in
//     fuse2's slot, then the BottleneckShift stages and the head as above (buf[4] and buf[1] rotate, buf[0] holds o).
int run_tdn(tsm_engine *e, Forward &f, const float *d_clips, int layout, int n_clips, float *d_logits, hipStream_t s) {
  const tsm_config &cfg = e->cfg;
  const bool seg_phase = layout == TSM_LAYOUT_TDN_SEGMENTS, ring_phase = layout == TSM_LAYOUT_TDN_RING;
  const int T = cfg.num_segments, n = seg_phase ? n_clips : n_clips * T, H = cfg.height, W = cfg.width, prec = e->prec;
  const int h5 = tdn_conv15_size(H), w5 = tdn_conv15_size(W);
  const int64_t plane = (int64_t)H * W, rows = (int64_t)h5 * w5;
  float *xc5 = f.t2;
  const int max_chunks = (cfg.max_clips + e->tdn_chunk - 1) / e->tdn_chunk;
  float *xd0 = e->buf[0], *stem = e->buf[4];
  if (ring_phase) {   // the trunk phase: nothing in front of fuse2 runs
    skip_slots(e, 2 * max_chunks + 3);
  } else {
    // (the segment phase: a segment is a clip of one segment -- e->tdn_pool is tdn_segments_pool's -- in chunks of as many frames)
    const int chunk_frames = e->tdn_chunk * T, seg_T = seg_phase ? 1 : T;
    int chunks = 0;
    for (int f0 = 0; f0 < n; f0 += chunk_frames, ++chunks) {
      const int nf = std::min(chunk_frames, n - f0);
      if (layout == TSM_LAYOUT_TDN_POOL || seg_phase) {
        TSM_LAUNCH(e, s, tsm::launch_tdn_front_pool(tdn_pool_source(e->tdn_pool, seg_T, f0 / seg_T), e->d_in4 + f0 * 4 * plane, e->d_patches, nf, H, W, s));
      } else {
        TSM_LAUNCH(e, s, tsm::launch_tdn_front(d_clips + f0 * kTdnPlanes * plane, e->d_in4 + f0 * 4 * plane, e->d_patches, nf, H, W, s));
      }
      // (the tuning pass times conv1_5's candidates on its first chunk only; a later, smaller chunk re-validates the code: checked_code)
      tsm::ConvParams p = make_params(e->convs[1], e->d_patches, nullptr, xc5 + f0 * rows * 64, nf, h5, w5, true, 0, 1, prec);
      const bool was_tuning = f.tuning;
      if (chunks > 0) f.tuning = false;
      const int rc = f.conv(1, p, 1, false);
      f.tuning = was_tuning;
      if (rc) return rc;
    }
    skip_slots(e, 2 * (max_chunks - chunks));
    if (f.want("diff.conv1_5")) return f.hit(xc5, n, h5, w5, 64);
    TSM_LAUNCH(e, s, tsm::launch_maxpool3x3s2(xc5, xd0, n, h5, w5, 64, prec, s));
    if (f.want("diff.stem")) return f.hit(xd0, n, e->hd, e->wd, 64);
    TSM_LAUNCH(e, s, tsm::launch_stem_pool(e->d_in4, e->convs[0].d_w, e->convs[0].d_b, stem, n, H, W, e->convs[0].kp, 1, prec, s, 0));
    if (f.want("stem")) return f.hit(stem, n, e->hp, e->wp, 64);
    TSM_LAUNCH(e, s, tsm::launch_tdn_fuse(stem, xd0, n, e->hp, e->wp, e->hd, e->wd, 64, e->tdn_alpha, e->tdn_beta, s));
    if (f.want("fuse1")) return f.hit(stem, n, e->hp, e->wp, 64);
  }

  const std::vector<BlockPlan> plan = f.tuning ? std::vector<BlockPlan>() : plan_forward(e, f.tiles, n, f.stage);
  float *cur = xd0, *out = e->buf[1], *xd1 = nullptr;
  int h = e->hd, w = e->wd;
  for (size_t k = 0; k < e->blocks.size(); ++k) {
    const Block &blk = e->blocks[k];
    const int conv_slots = (blk.down >= 0 ? 1 : 0) + 3;
    if (ring_phase && blk.mse < 0) {   // resnext_layer1 and layer1 ran in the segment phase
      skip_slots(e, conv_slots);
      continue;
    }
    if (seg_phase && blk.mse >= 0) {   // behind the seam: fuse2 (in front of the first BottleneckShift), the block's convs and its long-term module
      skip_slots(e, (blk.mse == 0 ? 1 : 0) + conv_slots + 5);
      continue;
    }
    if (!blk.diff_path && k > 0 && e->blocks[k - 1].diff_path) {   // the trunk starts: layer1 reads the blended stem
      xd1 = cur;
      f.obuf = xd1;   // (dead behind fuse2, which runs before the first BottleneckShift)
      out = xd1 == e->buf[0] ? e->buf[1] : e->buf[0];
      cur = stem;
      h = e->hp;
      w = e->wp;
    }
    if (blk.mse == 0) {   // the first BottleneckShift: layer1 is done
      if (ring_phase) {   // x from the ring, into the trunk's own buffers: buf[4] and buf[1] rotate, buf[0] holds o
        cur = stem;
        out = e->buf[1];
        f.obuf = e->buf[0];
        h = e->hp;
        w = e->wp;
        TSM_LAUNCH(e, s, tsm::launch_tdn_fuse_ring(e->tdn_ring.ring_a, e->tdn_ring.ring_d, e->tdn_ring.table, e->tdn_ring.n_slots, cur, n, h, w,
                                                   e->hd, e->wd, 256, e->tdn_alpha, e->tdn_beta, s));
      } else {
        TSM_LAUNCH(e, s, tsm::launch_tdn_fuse(cur, xd1, n, h, w, e->hd, e->wd, 256, e->tdn_alpha, e->tdn_beta, s));
      }
      if (f.want("fuse2")) return f.hit(cur, n, h, w, 256);
    }
    // the segment phase: the last block of resnext_layer1 and of layer1 write straight to the caller's out_d / out_a
    float *dst = out;
    if (seg_phase && (k + 1 == e->blocks.size() || e->blocks[k + 1].diff_path != blk.diff_path || e->blocks[k + 1].mse >= 0))
      dst = blk.diff_path ? e->tdn_seg.out_d : e->tdn_seg.out_a;
    const int rc = f.tuning ? f.tune_block(k, n, cur, dst, h, w) : f.run_block(k, plan[k], n, cur, dst, h, w);
    if (rc || f.tapped) return rc;
    if (dst == out) std::swap(cur, out);
    h = conv_out_size(h, 3, blk.stride);
    w = conv_out_size(w, 3, blk.stride);
  }
  if (seg_phase) {
    skip_slots(e, 1);   // the head
    return f.stage ? fail(e, TSM_ERR_INVALID_ARG, std::string("unknown stage: ") + f.stage) : (int)TSM_OK;
  }
  return run_head(e, cur, n, n_clips, h * w, d_logits, s, f.stage);
}

// The tile-cache key of a call: the bucket's frame count; the two phases of a TDN forward keep buckets of their own
// (tsm_host_util.h: kTdnSegmentsKey / kTdnRingKey), so a phase that tunes only its own convs never stands in for a whole forward.
int tune_key_of(const tsm_engine *e, int layout, int n_clips) {
  if (layout == TSM_LAYOUT_TDN_SEGMENTS) return kTdnSegmentsKey + tile_bucket(n_clips);
  if (layout == TSM_LAYOUT_TDN_RING) return kTdnRingKey + tile_bucket(n_clips) * e->cfg.num_segments;
  return tile_bucket(n_clips) * e->cfg.num_segments;
}

// Enqueue the forward on `s`.  If `stage` is non-null, stop right after that stage and report it.
int run_forward(tsm_engine *e, const float *d_clips, int layout, int n_clips, float *d_logits,
                hipStream_t s, const char *stage, Tap *tap) {
  const tsm_config &cfg = e->cfg;
  const int T = cfg.num_segments;
  int n = n_clips * T;   // (a temporal-pool engine halves it behind layer1)
  Forward f(e, s, stage, tap);
  // Tile shape per conv layer for this frame count: tuned on first use by timing every valid shape on
  // the real launch (all shapes give bit-identical results: the k order per output does not depend on
  // the tile), then cached.  TSM_AUTOTUNE=0 keeps the static heuristic.
  if (e->autotune && !stage) {
    const int key = tune_key_of(e, layout, n_clips);
    auto it = e->tile_cache.find(key);
    if (it == e->tile_cache.end()) {
      it = e->tile_cache.emplace(key, std::vector<int>(e->convs.size(), 0)).first;
      f.tuning = true;
    }
    f.tiles = &it->second;
  }
  if (e->convnext) return run_convnext(e, f, d_clips, layout, n, d_logits, s);
  if (e->tdn) return run_tdn(e, f, d_clips, layout, n_clips, d_logits, s);

  const int prec = e->prec;
  const float *in4 = e->d_in4;
  // The pool-fused stem reads the reference layout ([N, T, 3, H, W] fp32) itself and converts while it stages its patch:
  // no pack launch, no packed copy (TSM_STEM_PLANAR=0 and every other stem form keep the pack; all bit-identical).
  const bool pool_stem = e->stem_direct && e->stem_pool && !f.want("conv1");
  // (8-byte loads of pixel pairs: a caller's pointer that is only 4-byte aligned takes the pack launch, which loads floats)
  const bool planar = layout == TSM_LAYOUT_NTCHW && e->stem_planar && pool_stem && !f.want("input") &&
                      (double)cfg.height * cfg.width * 12.0 < 2.0e9 && (reinterpret_cast<uintptr_t>(d_clips) & 15u) == 0;
  if (layout >= TSM_LAYOUT_NTHWC4 || planar) {
    in4 = d_clips;      // already packed by tsm_preprocess (or read as it is by the stem): consumed in place
    skip_slots(e, 1);   // the pack
  } else {
    TSM_LAUNCH(e, s, tsm::launch_pack_input(d_clips, e->d_in4, n, cfg.height, cfg.width,
                                            layout == TSM_LAYOUT_NTCHW ? 1 : 0, prec, s));
  }
  if (f.want("input"))  // fp32: [n,H,W,4]; bf16 formats: pixel pairs [n,H,ceil(W/2),8]
    return prec == tsm::kPrecF32 ? f.hit(in4, n, cfg.height, cfg.width, 4) : f.hit(in4, n, cfg.height, (cfg.width + 1) / 2, 8);

  float *cur = e->buf[0], *out = e->buf[1], *t1 = f.t1;
  {
    tsm::ConvParams p = make_params(e->convs[0], in4, nullptr, t1, n, cfg.height, cfg.width, true, 0, 1, prec);
    // bf16 formats: dedicated direct-conv stem (LDS-resident input patch), with the max-pool fused behind it unless
    // the un-pooled tensor itself is wanted; TSM_STEM_DIRECT=0 / TSM_STEM_POOL=0 fall back (all forms bit-identical)
    const bool direct = prec != tsm::kPrecF32 && e->stem_direct;   // (fp32 has the pool-fused direct form only)
    if (pool_stem) {
      TSM_LAUNCH(e, s, tsm::launch_stem_pool(in4, e->convs[0].d_w, e->convs[0].d_b, cur, n, cfg.height, cfg.width,
                                              e->convs[0].kp, 1, prec, s, planar ? 1 : 0));
      skip_slots(e, 1);   // the max-pool
    } else {
      if (direct) {
        TSM_LAUNCH(e, s, tsm::launch_stem_direct(in4, e->convs[0].d_w, e->convs[0].d_b, t1, n, cfg.height, cfg.width,
                                                  e->convs[0].kp, 1, prec, s));
      } else {
        int rc0 = f.conv(0, p, 7, false);
        if (rc0) return rc0;
      }
      if (f.want("conv1")) return f.hit(t1, n, e->h1, e->w1, 64);
      TSM_LAUNCH(e, s, tsm::launch_maxpool3x3s2(t1, cur, n, e->h1, e->w1, 64, prec, s));
    }
    if (f.want("stem")) return f.hit(cur, n, e->hp, e->wp, 64);
  }
  int h = e->hp, w = e->wp;
  const std::vector<BlockPlan> plan = f.tuning ? std::vector<BlockPlan>() : plan_forward(e, f.tiles, n, stage);
  for (size_t k = 0; k < e->blocks.size(); ++k) {
    const int rc = e->blocks[k].conv3 < 0 ? f.run_basic(k, n, cur, out, h, w)
                   : f.tuning            ? f.tune_block(k, n, cur, out, h, w)
                                         : f.run_block(k, plan[k], n, cur, out, h, w);
    if (rc || f.tapped) return rc;
    std::swap(cur, out);
    h = conv_out_size(h, 3, e->blocks[k].stride);
    w = conv_out_size(w, 3, e->blocks[k].stride);
    if (e->blocks[k].nl_qkv >= 0) {   // the wrapper: the block's output (now cur) -> z in the block's dead input buffer
      const int rcn = f.run_nonlocal(k, n, cur, out, h, w);
      if (rcn || f.tapped) return rcn;
      std::swap(cur, out);
    }
    if (e->blocks[k].tpool_after) {   // the temporal pool: layer1's output (cur) -> T / 2 frames per clip in the dead buffer
      const Block &blk = e->blocks[k];
      const int c = e->convs[blk.conv3 >= 0 ? blk.conv3 : blk.conv2].cout;
      TSM_LAUNCH(e, s, tsm::launch_temporal_maxpool(cur, out, n_clips, T, (int64_t)h * w, c, prec, s));
      std::swap(cur, out);
      n /= 2;
      if (f.want("layer2.tpool")) return f.hit(cur, n, h, w, c);
    }
  }
  return run_head(e, cur, n, n_clips, h * w, d_logits, s, stage);
}

// The tile codes of the bucket `n_clips` falls into: already in memory, read from the tune cache file, or timed now on
// the real launches over `d_clips` (synchronises; the codes then go to the cache file).
int ensure_tuned(tsm_engine *e, const float *d_clips, int layout, int n_clips, float *d_out, hipStream_t s,
                 bool *from_file = nullptr) {
  const int tune_key = tune_key_of(e, layout, n_clips);
  if (from_file) *from_file = false;
  if (!e->autotune || e->tile_cache.find(tune_key) != e->tile_cache.end()) return TSM_OK;
  std::vector<int> cached(e->convs.size(), 0);
  if (tune_cache_load(e, tune_key, &cached)) {
    e->tile_cache.emplace(tune_key, cached);          // tuned by an earlier process (TSM_TUNE_CACHE)
    if (from_file) *from_file = true;
    return TSM_OK;
  }
  std::vector<hipEvent_t> *saved = e->cur_timing;
  e->cur_timing = nullptr;
  const int rc = run_forward(e, d_clips, layout, n_clips, d_out, s, nullptr, nullptr);
  e->cur_timing = saved;
  if (rc) return rc;
  tune_cache_store(e, tune_key, e->tile_cache[tune_key]);
  return TSM_OK;
}

// Device-memory calls run where the caller's data lives: `stream`, NULL meaning the device's default
// (null) stream -- which is what torch's default stream is.  Host-memory calls are synchronous and use
// the engine's private stream unless one is given.
hipStream_t pick_stream(tsm_engine *e, int memkind, void *stream) {
  if (stream) return static_cast<hipStream_t>(stream);
  return memkind == TSM_MEM_HOST ? e->stream : nullptr;
}

// Tuned codes of one backbone or placement are never read by another: " r<depth>" for a backbone other than R50, " w<width>"
// for a wide one, " block" for block placement (an R50 blockres engine keeps the bare signature, so existing cache lines stay
// valid).
void retag_tune_sig(tsm_engine *e) {
  if (e->tune_sig.empty()) return;
  e->tune_sig.resize(e->tune_sig_base);
  if (e->depth != 50) e->tune_sig += " r" + std::to_string(e->depth);
  if (e->width != 64) e->tune_sig += " w" + std::to_string(e->width);
  if (e->place == 1) e->tune_sig += " block";
  if (e->convnext) {
    e->tune_sig += " cnx";
    for (int s = 0; s < kCnxStages; ++s) e->tune_sig += (s ? "-" : "") + std::to_string(e->cnx_depths[s]);
  }
  if (e->tdn) {
    e->tune_sig += " tdn";
    for (int s = 0; s < 4; ++s) e->tune_sig += (s ? "-" : "") + std::to_string(e->tdn_depths[s]);
  }
  if (e->non_local) e->tune_sig += " nl";
  if (e->temporal_pool) e->tune_sig += " tp";
}

int check_forward_args(tsm_engine *e, const void *clips, int memkind, int layout, int n_clips) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (!e->finalized) return fail(e, TSM_ERR_NOT_FINALIZED, "tsm_finalize has not been called");
  if (!clips) return fail(e, TSM_ERR_INVALID_ARG, "clips is NULL");
  if (memkind != TSM_MEM_HOST && memkind != TSM_MEM_DEVICE) return fail(e, TSM_ERR_INVALID_ARG, "bad memkind");
  if ((layout < TSM_LAYOUT_NTCHW || layout > TSM_LAYOUT_NTHWC8B) && (layout < TSM_LAYOUT_TDN_POOL || layout > TSM_LAYOUT_TDN_RING))
    return fail(e, TSM_ERR_INVALID_ARG, "bad layout");
  if (layout == TSM_LAYOUT_TDN_SEGMENTS || layout == TSM_LAYOUT_TDN_RING) {   // `clips` is a descriptor in host memory, as below
    const bool seg = layout == TSM_LAYOUT_TDN_SEGMENTS;
    if (!e->tdn) return fail(e, TSM_ERR_UNSUPPORTED, "TSM_LAYOUT_TDN_SEGMENTS / TSM_LAYOUT_TDN_RING go with a TDN engine (tsm_set_tdn) only");
    if (memkind != TSM_MEM_DEVICE) return fail(e, TSM_ERR_INVALID_ARG, "the phases of a TDN forward name device memory: memkind must be TSM_MEM_DEVICE");
    const char *why = seg ? tdn_segments_refusal(static_cast<const tsm_tdn_segments *>(clips)) : tdn_ring_refusal(static_cast<const tsm_tdn_ring *>(clips));
    if (why) return fail(e, TSM_ERR_INVALID_ARG, why);
    if (seg) {   // n_clips counts segments
      const int64_t cap = (int64_t)e->cfg.max_clips * e->cfg.num_segments;
      if (n_clips <= 0) return fail(e, TSM_ERR_INVALID_ARG, "the segment count must be positive");
      if (n_clips > cap) return fail(e, TSM_ERR_CAPACITY, "segment count " + std::to_string(n_clips) + " exceeds max_clips * T = " + std::to_string(cap));
      return TSM_OK;
    }
  } else if (layout == TSM_LAYOUT_TDN_POOL) {   // `clips` is a tsm_tdn_pool in host memory: checked and copied here, nothing of it is read later
    if (!e->tdn) return fail(e, TSM_ERR_UNSUPPORTED, "TSM_LAYOUT_TDN_POOL goes with a TDN engine (tsm_set_tdn) only");
    if (memkind != TSM_MEM_DEVICE) return fail(e, TSM_ERR_INVALID_ARG, "TSM_LAYOUT_TDN_POOL names frames in device memory: memkind must be TSM_MEM_DEVICE");
    if (const char *why = tdn_pool_refusal(static_cast<const tsm_tdn_pool *>(clips))) return fail(e, TSM_ERR_INVALID_ARG, why);
  } else if (e->tdn && layout != TSM_LAYOUT_NTCHW) {
    return fail(e, TSM_ERR_UNSUPPORTED, "a TDN engine takes TSM_LAYOUT_NTCHW only: [n_clips, T, 15, H, W], five frames per segment (or TSM_LAYOUT_TDN_POOL)");
  }
  const bool packed = layout >= TSM_LAYOUT_NTHWC4 && layout <= TSM_LAYOUT_NTHWC8B;
  if (packed && memkind != TSM_MEM_DEVICE)
    return fail(e, TSM_ERR_INVALID_ARG, "packed layouts (NTHWC4 / NTHWC8S / NTHWC8B) are device-memory layouts");
  if (packed && layout != packed_layout_of(e->prec))
    return fail(e, TSM_ERR_INVALID_ARG, "packed layout does not match the engine dtype");
  if (n_clips <= 0) return fail(e, TSM_ERR_INVALID_ARG, "n_clips must be positive");
  if (n_clips > e->cfg.max_clips)
    return fail(e, TSM_ERR_CAPACITY, "n_clips " + std::to_string(n_clips) + " exceeds max_clips " +
                                         std::to_string(e->cfg.max_clips));
  return TSM_OK;
}

// Behind check_forward_args: the engine's device, the call's stream, and clips in host memory staged into d_in.
int stage_input(tsm_engine *e, const void *clips, int memkind, int layout, int n_clips, void *stream, hipStream_t *s, const float **d_clips) {
  TSM_HIP(e, hipSetDevice(e->cfg.device_id));
  *s = pick_stream(e, memkind, stream);
  *d_clips = static_cast<const float *>(clips);
  if (layout == TSM_LAYOUT_TDN_POOL) {   // (behind tdn_pool_refusal) the forward reads e->tdn_pool, never `clips`
    e->tdn_pool = *static_cast<const tsm_tdn_pool *>(clips);
    *d_clips = nullptr;
  } else if (layout == TSM_LAYOUT_TDN_SEGMENTS) {   // (behind tdn_segments_refusal)
    e->tdn_seg = *static_cast<const tsm_tdn_segments *>(clips);
    e->tdn_pool = tdn_segments_pool(e->tdn_seg);
    *d_clips = nullptr;
  } else if (layout == TSM_LAYOUT_TDN_RING) {       // (behind tdn_ring_refusal)
    e->tdn_ring = *static_cast<const tsm_tdn_ring *>(clips);
    *d_clips = nullptr;
  }
  if (memkind == TSM_MEM_HOST) {
    const size_t in_elems = (size_t)n_clips * e->cfg.num_segments * (e->tdn ? kTdnPlanes : 3) * e->cfg.height * e->cfg.width;
    TSM_HIP(e, hipMemcpyAsync(e->d_in, clips, in_elems * sizeof(float), hipMemcpyHostToDevice, *s));
    *d_clips = e->d_in;
  }
  return TSM_OK;
}

// The backbone, the placement and the consensus are fixed once weights arrive.
int check_before_weights(tsm_engine *e, const char *setter) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (e->weights_started || e->finalized) return fail(e, TSM_ERR_INVALID_ARG, std::string(setter) + " must come before the first tsm_set_tensor");
  return TSM_OK;
}

// The ResNet setters on a ConvNeXt engine (tsm_set_convnext came first): refused, the topology has none of their parts.
int refuse_on_convnext(tsm_engine *e, const char *setter) {
  if (e->tdn) return fail(e, TSM_ERR_UNSUPPORTED, std::string(setter) + ": a TDN engine (tsm_set_tdn) has no such part");
  if (!e->convnext) return TSM_OK;
  return fail(e, TSM_ERR_UNSUPPORTED, std::string(setter) + ": a ConvNeXt engine (tsm_set_convnext) has no such part");
}

// tsm_finalize's weight allocations: dev_alloc under the name "weights", no frame.
struct WeightAlloc {
  tsm_engine *e;
  int operator()(float **p, const char *, size_t elems, size_t) const { return dev_alloc(e, p, elems); }
};

// The four vectors of BatchNorm `bnp` side by side: [gamma | beta | mean | var], c each.
std::vector<float> batchnorm(const tsm_engine *e, const std::string &bnp) {
  std::vector<float> bn;
  for (int i = 0; i < 4; ++i) {
    const std::vector<float> &v = tensor(e, bnp + kBnSuffix[i]);
    bn.insert(bn.end(), v.begin(), v.end());
  }
  return bn;
}

// Conv c's host tensors -> the folded fp32 matrix [cout][kp] in c's geometry and the bias, as its kind packs them
// (tsm_host_util.h: fold_and_pack*, cnx_pack_*, cnx_fold_gamma, tdn_*).
void pack_conv(const tsm_engine *e, const ConvLayer &c, std::vector<float> *wp, std::vector<float> *bias) {
  const float *w = tensor(e, c.wkey).data();
  const std::vector<float> bn = c.bnp.empty() ? std::vector<float>() : batchnorm(e, c.bnp);
  const float *g = nullptr, *b = nullptr, *m = nullptr, *v = nullptr;
  if (!bn.empty()) { g = bn.data(); b = g + c.cout; m = b + c.cout; v = m + c.cout; }
  auto conv_bias = [&]() -> const std::vector<float> & { return tensor(e, bias_key(c.wkey)); };
  switch (c.kind) {
    case ConvKind::kBn: prepare_weights(c, w, g, b, m, v, wp, bias); break;
    case ConvKind::kNlQkv:
    case ConvKind::kNlW: {   // [cout, cin, 1, 1, 1] weights with a bias; theta | phi | g concatenated along cout
      const int parts = c.kind == ConvKind::kNlQkv ? 3 : 1, pc = c.cout / parts;
      wp->assign((size_t)c.cout * c.kp, 0.f);
      bias->assign(c.cout, 0.f);
      for (int part = 0; part < parts; ++part) {
        const std::string wkey = parts == 3 ? c.nlp + kNlQkv[part] + ".weight" : c.wkey;
        fold_and_pack_bias(tensor(e, wkey).data(), tensor(e, bias_key(wkey)).data(), g, b, m, v, pc, c.cin, c.kp, part * pc, wp, bias);
      }
      break;
    }
    case ConvKind::kCnxStem: cnx_pack_stem(w, c.cout, wp); *bias = conv_bias(); break;
    case ConvKind::kCnxDown: cnx_pack_down(w, c.cout, c.cin / 4, wp); *bias = conv_bias(); break;
    case ConvKind::kCnxFc1: *wp = tensor(e, c.wkey); *bias = conv_bias(); break;
    case ConvKind::kCnxFc2: cnx_fold_gamma(w, conv_bias().data(), tensor(e, c.gkey).data(), c.cout, c.cin, wp, bias); break;
    case ConvKind::kTdnBias: {
      const std::vector<float> mean = tdn_mean_less_bias(m, conv_bias().data(), c.cout);
      prepare_weights(c, w, g, b, mean.data(), v, wp, bias);
      break;
    }
    case ConvKind::kTdnConv15: tdn_pack_conv15(w, g, b, m, v, c.cout, wp, bias); break;
  }
}

// One affine pair "<key>.weight" / "<key>.bias" as it is: a LayerNorm's, the classifier's.
int upload_pair(tsm_engine *e, WeightAlloc &alloc, const std::string &key, float **d_w, float **d_b, const char *wname, const char *bname) {
  const int rc = upload(e, alloc, d_w, wname, tensor(e, key + ".weight"));
  return rc ? rc : upload(e, alloc, d_b, bname, tensor(e, key + ".bias"));
}

// A ConvNeXt engine's tensors outside its GEMMs: the LayerNorm pairs and every block's depthwise conv (cnx_pack_dw).
int upload_convnext_norms_and_dw(tsm_engine *e, WeightAlloc &alloc) {
  auto upload_norm = [&](CnxNorm &n) { return upload_pair(e, alloc, n.key, &n.d_w, &n.d_b, "ln_w", "ln_b"); };
  if (int rc = upload_norm(e->cnx_stem_norm)) return rc;
  if (int rc = upload_norm(e->cnx_head_norm)) return rc;
  for (CnxStage &st : e->cnx_stages)
    if (st.down >= 0)
      if (int rc = upload_norm(st.norm)) return rc;
  for (CnxBlock &blk : e->cnx_blocks) {
    std::vector<float> wp;
    cnx_pack_dw(tensor(e, blk.dwkey + ".weight").data(), blk.c, &wp);
    if (int rc = upload(e, alloc, &blk.d_dw, "dw_w", wp)) return rc;
    if (int rc = upload(e, alloc, &blk.d_dwb, "dw_b", tensor(e, blk.dwkey + ".bias"))) return rc;
    if (int rc = upload_norm(blk.norm)) return rc;
  }
  return TSM_OK;
}

// A TDN engine's long-term modules, one per BottleneckShift (tdn_pack_mse).
int upload_tdn_mse(tsm_engine *e, WeightAlloc &alloc) {
  for (TdnMse &m : e->tdn_mse) {
    const float *conv[kMseConvs];
    std::vector<float> bn[kMseBns];
    for (int i = 0; i < kMseConvs; ++i) conv[i] = tensor(e, m.key + kTdnMseConvs[i]).data();
    for (int i = 0; i < kMseBns; ++i) bn[i] = batchnorm(e, m.key + kTdnMseBns[i]);
    TdnMseWeights pk;
    tdn_pack_mse(m.c, conv[kMseConv1], bn[kMseBn1].data(), conv[kMseConv2], conv[kMseSmall2], bn[kMseBnSmall2].data(), conv[kMseSmall4],
                 bn[kMseBnSmall4].data(), conv[kMseConv3], bn[kMseBn3].data(), conv[kMseTemporal], &pk);
    const std::pair<float **, const std::vector<float> *> parts[] = {
        {&m.d_wq, &pk.wq}, {&m.d_bq, &pk.bq}, {&m.d_dw, &pk.dw}, {&m.d_k2, &pk.k2}, {&m.d_b2, &pk.b2},
        {&m.d_k4, &pk.k4}, {&m.d_b4, &pk.b4}, {&m.d_w3, &pk.w3}, {&m.d_b3, &pk.b3}, {&m.d_wt, &pk.wt}};
    for (const auto &part : parts)
      if (int rc = upload(e, alloc, part.first, "mse_w", *part.second)) return rc;
  }
  return TSM_OK;
}

// The Bottleneck fusions' weights, from the folded fp32 matrices of the 1x1 layers (host_wp / host_bias by conv index), for
// the ResNet and TDN engines alike.
template <class Alloc>
int upload_block_fusions(tsm_engine *e, Alloc &alloc, const std::vector<std::vector<float>> &host_wp, const std::vector<std::vector<float>> &host_bias) {
  // First block of every stage: out = relu(conv3(h2) + downsample(x)) as one GEMM, K concatenated.
  for (Block &blk : e->blocks) {
    if (blk.down < 0 || blk.conv3 < 0) continue;   // (Bottlenecks only)
    const ConvLayer &c3 = e->convs[blk.conv3], &cd = e->convs[blk.down];
    std::vector<float> wf, bf;
    concat_k_pair(host_wp[blk.conv3], host_bias[blk.conv3], c3.kp, host_wp[blk.down], host_bias[blk.down], cd.kp, c3.cout,
                  &wf, &bf);
    if (int rc = upload_conv(e, alloc, e->prec, c3.cout, &wf, bf, &blk.d_wf, &blk.d_bf)) return rc;
  }
  // Blocks without a downsample branch whose mid tensor is 64 / 128 channels wide and whose conv3 has 4x as many outputs
  // (conv23_fused_kernel: four phase-C chunks), or 128 wide with 2x as many (conv23_fused2_kernel, wide_resnet50_2's
  // layer1.1-2: two chunks): conv3's weights once more, in the fragment order of the fused conv2 + conv3 kernel (fp32 and
  // split-bf16 engines).  Any other mid / output pair keeps the two separate launches.
  for (Block &blk : e->blocks) {
    if (blk.conv3 < 0) continue;   // (Bottlenecks only)
    const ConvLayer &c2 = e->convs[blk.conv2], &c3 = e->convs[blk.conv3];
    if (blk.down >= 0 || blk.stride != 1 || (c2.cout != 64 && c2.cout != 128)) continue;
    if (e->prec == tsm::kPrecBf16) {   // weight-stationary form: 64 mid channels only; it reads conv3's packed matrix itself
      if (c2.cout == 64 && c2.cin == 64 && c3.cout == 256) { blk.cmid = 64; blk.cout3 = 256; }
      continue;
    }
    const int nchunk = c3.cout == 4 * c2.cout ? 4 : (c3.cout == 2 * c2.cout && c2.cout == 128) ? 2 : 0;
    if (nchunk == 0) continue;
    std::vector<float> w3f;
    if (e->prec == tsm::kPrecBf16x3) pack_w3_fragments_split(host_wp[blk.conv3].data(), c2.cout, &w3f, nchunk);
    else pack_w3_fragments(host_wp[blk.conv3].data(), c2.cout, &w3f, nchunk);
    if (int rc = upload(e, alloc, &blk.d_w3f, "d_w3f", w3f)) return rc;
    blk.cmid = c2.cout;
    blk.cout3 = c3.cout;
  }
  return TSM_OK;
}

// Floats of the largest activation of one frame of a ResNet or TDN engine: `start` (the stem conv's output; a TDN engine's x_c5
// and layer1 on the stem's pooled map) or a conv output of some block (R50: layer1's 256 channels).  *mse_frame: the largest
// r-channel map of a TDN long-term module.  The walk starts again on the difference path's maps where a TDN engine changes path.
size_t activation_frame_elems(const tsm_engine *e, size_t start, size_t *mse_frame) {
  size_t per_frame = start;
  *mse_frame = 0;
  int hh = 0, ww = 0;
  for (size_t k = 0; k < e->blocks.size(); ++k) {
    const Block &blk = e->blocks[k];
    if (k == 0 || blk.diff_path != e->blocks[k - 1].diff_path) {
      hh = blk.diff_path ? e->hd : e->hp;
      ww = blk.diff_path ? e->wd : e->wp;
    }
    const size_t in_px = (size_t)hh * ww;
    if (blk.mse >= 0) *mse_frame = std::max(*mse_frame, in_px * (size_t)(e->tdn_mse[blk.mse].c / kTdnReduction));
    hh = conv_out_size(hh, 3, blk.stride);
    ww = conv_out_size(ww, 3, blk.stride);
    const size_t out_px = (size_t)hh * ww;
    for (int ci : {blk.conv1, blk.conv2, blk.conv3, blk.down}) {
      if (ci < 0) continue;
      // (a Bottleneck's conv1 runs at the block input's size, every other conv at the block output's)
      const bool at_input = blk.conv3 >= 0 && ci == blk.conv1;
      per_frame = std::max(per_frame, (at_input ? in_px : out_px) * (size_t)e->convs[ci].cout);
    }
    // (a non-local engine only: theta | phi | g of a wrapped block, 3 d channels at the block's output size)
    if (blk.nl_qkv >= 0) per_frame = std::max(per_frame, out_px * (size_t)e->convs[blk.nl_qkv].cout);
  }
  return per_frame;
}

// What alloc_workspace sizes the buffers from, in floats.
struct Workspace {
  size_t frames = 0;        // max_clips * num_segments
  size_t per_frame = 0;     // the largest activation of one frame
  size_t in_frame = 0;      // one input frame as a host caller hands it over (d_in) ...
  size_t in4_frame = 0;     // ... and packed (d_in4)
  // a TDN engine: conv1_5's patch rows of one frame and the frames of one front-end chunk; the long-term modules' largest map
  size_t patch_frame = 0, patch_frames = 0, mse_frame = 0;
};

// The workspace of every family: five rotating buffers (block in / out, two branch temporaries, identity), each the largest
// activation of the schedule; the input staging and packing buffers; a TDN engine's patch rows and its nine r-channel maps; the
// head's buffers; the split-K scratch of an fp32 engine.  Then the host copies go and the engine is finalized.
int alloc_workspace(tsm_engine *e, const Workspace &ws) {
  const tsm_config &cfg = e->cfg;
  int rc;
  e->buf_elems = ws.frames * ws.per_frame;
  for (int i = 0; i < 5; ++i) {
    static const char *const kBufNames[5] = {"buf[0]", "buf[1]", "buf[2]", "buf[3]", "buf[4]"};
    if ((rc = dev_alloc(e, &e->buf[i], e->buf_elems, kBufNames[i], ws.per_frame))) return rc;
  }
  if ((rc = dev_alloc(e, &e->d_in, ws.frames * ws.in_frame, "d_in", ws.in_frame))) return rc;
  if ((rc = dev_alloc(e, &e->d_in4, ws.frames * ws.in4_frame, "d_in4", ws.in4_frame))) return rc;
  if (ws.patch_frame) {
    if ((rc = dev_alloc(e, &e->d_patches, ws.patch_frames * ws.patch_frame, "d_patches", ws.patch_frame))) return rc;
    static const char *const kMseNames[9] = {"mse.b", "mse.d+", "mse.d-", "mse.m+", "mse.m-", "mse.pool+", "mse.pool-", "mse.s2+", "mse.s2-"};
    for (int i = 0; i < 9; ++i)   // (the pooled maps are a quarter of the size at most; one size for all keeps the bands' frame)
      if ((rc = dev_alloc(e, &e->d_mse[i], ws.frames * ws.mse_frame, kMseNames[i], ws.mse_frame))) return rc;
  }
  if ((rc = dev_alloc(e, &e->d_pooled, ws.frames * (size_t)e->feat, "d_pooled", (size_t)e->feat))) return rc;
  // avg: one row per clip; identity: one per (clip, segment)
  if ((rc = dev_alloc(e, &e->d_logits, (size_t)cfg.max_clips * (e->consensus == 1 ? out_segments(e) : 1) * cfg.num_class, "d_logits",
                      (size_t)cfg.num_class))) return rc;
  if (e->prec == tsm::kPrecF32) {  // split-K scratch: 64 MB covers the small-batch cases where split-K can win
    e->partial_elems = (size_t)16 << 20;
    if ((rc = dev_alloc(e, &e->d_partial, e->partial_elems, "d_partial", ws.per_frame))) return rc;
  }
  e->tensors.clear();  // host copies are no longer needed
  e->finalized = true;
  return TSM_OK;
}

// A TSM_* variable of tsm_create: *v keeps its default when the variable is unset.
template <class T, class F>
void env_read(const char *name, T *v, F parse) { if (const char *s = getenv(name)) *v = parse(s); }

// tsm_conv_op's temporaries.  Hostile memory, always on (a debug entry point that allocates per call): every temporary sits
// between poisoned bands of one frame of that buffer and starts out poison all over -- so the elements of d_ys / d_part that the
// launch does not write reach y as poison (through to_f32 / the reduction), a read before frame 0 or behind the last tile returns
// poison instead of the allocator's leftovers, and a stray store is found in the bands after the final synchronise
// (TSM_ERR_GUARD).  Freed on every exit path (errors included).
struct GuardedScratch {
  GuardBuf g[8];
  int n = 0;
  ~GuardedScratch() {
    for (int i = 0; i < n; ++i)
      if (g[i].base) (void)hipFree(g[i].base);
  }
  int alloc(float **p, const char *name, size_t elems, size_t frame_elems, size_t elem_bytes = 4) {
    GuardBuf &b = g[n++];
    TSM_HIP(nullptr, guard_alloc(&b, name, elems * elem_bytes, frame_elems * elem_bytes, elem_bytes));
    *p = b.ptr();
    return TSM_OK;
  }
};

// tsm_conv_op: layer c's raw OIHW weights and BatchNorm vectors copied from device memory, then prepare_weights.
int fetch_prepared(const ConvLayer &c, const float *w, const float *gamma, const float *beta, const float *mean, const float *var,
                   std::vector<float> *wp, std::vector<float> *bias) {
  const size_t nw = (size_t)c.cout * c.cin * c.k * c.k, nc = (size_t)c.cout;
  std::vector<float> host(nw + 4 * nc);
  const float *src[5] = {w, gamma, beta, mean, var};
  float *dst = host.data();
  for (int i = 0; i < 5; ++i) {   // [raw weights | gamma | beta | mean | var]
    TSM_HIP(nullptr, hipMemcpy(dst, src[i], (i ? nc : nw) * sizeof(float), hipMemcpyDeviceToHost));
    dst += i ? nc : nw;
  }
  const float *bn = host.data() + nw;
  prepare_weights(c, host.data(), bn, bn + nc, bn + 2 * nc, bn + 3 * nc, wp, bias);
  return TSM_OK;
}

// The status of an engine-less entry point's launch: `op`: and HIP's text, or for hipErrorInvalidValue -- the launchers'
// "these arguments fit no launch" -- `invalid_text` where the entry point has a better one.
int op_status(const char *op, hipError_t st, const char *invalid_text = nullptr) {
  if (st == hipSuccess) return TSM_OK;
  const int code = st == hipErrorInvalidValue ? TSM_ERR_INVALID_ARG : TSM_ERR_HIP;
  return fail(nullptr, code, std::string(op) + ": " + (invalid_text && code == TSM_ERR_INVALID_ARG ? invalid_text : hipGetErrorString(st)));
}

}  // namespace

// ---- the frame transforms (tsm_preprocess, _clips, _indexed, _windows, _image): their shared argument checks ----------------------------
static int out_mode_of(int32_t out_layout, int *mode) {          // PreprocParams::out_mode of an output layout; any other is refused
  *mode = out_layout == TSM_LAYOUT_NTHWC4 ? 0 : out_layout == TSM_LAYOUT_NTCHW ? 1 : out_layout == TSM_LAYOUT_NTHWC8S ? 2 : out_layout == TSM_LAYOUT_NTHWC8B ? 3 : -1;
  return *mode >= 0 ? TSM_OK : fail(nullptr, TSM_ERR_INVALID_ARG, "out_layout must be NTHWC4, NTHWC8S, NTHWC8B or NTCHW");
}
// The pixel type, output layout and scale of a frame transform, checked and written into its parameter block.
template <typename P>
static int set_pixel_format(P *p, int32_t pixel, int32_t out_layout, int32_t scale_255) {
  tsm_host::Nv12Coef k{};
  p->src_yuv = tsm_host::nv12_coefficients(pixel, &k) ? 1 : tsm_host::yuv_coefficients(pixel, &k) ? 2 + tsm_host::yuv_layout_of(pixel) : 0;
  if (pixel != TSM_PIXEL_U8 && pixel != TSM_PIXEL_F32 && !p->src_yuv) return fail(nullptr, TSM_ERR_INVALID_ARG, "bad pixel type");
  if (int rc = out_mode_of(out_layout, &p->out_mode)) return rc;
  p->src_is_u8 = pixel == TSM_PIXEL_U8;
  const int32_t words[tsm_host::kNv12CoefWords] = {k.y_off, k.cy, k.crv, k.cgu, k.cgv, k.cbu};
  memcpy(p->nv12, words, sizeof words);
  p->pre_scale = scale_255 ? 1.0f / 255.0f : 1.0f;
  return TSM_OK;
}
// YUV frames of a launch whose frame size is an argument.  NV12: both sides even, the buffer 2-byte aligned.  The other
// formats: the parity and the alignment of their layout (tsm_host::yuv_sides_ok, yuv_alignment).
static int check_yuv_frames(const char *op, int32_t pixel, const void *frames, int h, int w) {
  const int layout = tsm_host::yuv_layout_of(pixel);
  if (layout >= 0) {
    static const char *const names[tsm_host::kYuvLayouts] = {"I420", "YV12", "P010", "YUYV", "UYVY"};
    const std::string what = std::string(op) + ": " + names[layout] + " frames ";
    if (!tsm_host::yuv_sides_ok(layout, h, w))
      return fail(nullptr, TSM_ERR_INVALID_ARG, what + (tsm_host::yuv_is_420(layout) ? "need an even h and an even w, got " : "need an even w, got ") +
                                                    std::to_string(h) + " x " + std::to_string(w));
    const int align = tsm_host::yuv_alignment(layout);
    if (reinterpret_cast<uintptr_t>(frames) & (uintptr_t)(align - 1))
      return fail(nullptr, TSM_ERR_INVALID_ARG, what + "must be " + std::to_string(align) + "-byte aligned");
    return TSM_OK;
  }
  if (!tsm_host::pixel_is_nv12(pixel)) return TSM_OK;
  if ((h | w) & 1)
    return fail(nullptr, TSM_ERR_INVALID_ARG, std::string(op) + ": NV12 frames need an even h and an even w, got " + std::to_string(h) + " x " + std::to_string(w));
  if (reinterpret_cast<uintptr_t>(frames) & 1) return fail(nullptr, TSM_ERR_INVALID_ARG, std::string(op) + ": NV12 frames must be 2-byte aligned");
  return TSM_OK;
}
// Resize(resize) + CenterCrop(crop) of an h x w frame into a PreprocParams / ImagePreprocParams (tsm_host::center_crop_geometry);
// false when the crop is larger than the resized frame.
template <typename P>
static bool set_crop_geometry(P *p, int h, int w, int resize, int crop) {
  tsm_host::CropGeometry g;
  if (!tsm_host::center_crop_geometry(h, w, resize, crop, &g)) return false;
  p->h = h; p->w = w; p->nh = g.nh; p->nw = g.nw; p->top = g.top; p->left = g.left; p->crop = crop;
  return true;
}

extern "C" {

int tsm_abi_version(void) { return TSM_ABI_VERSION; }

const char *tsm_build_id(void) { return kBuildTag + sizeof("tsm-build-id:") - 1; }

int tsm_trace_launches(int32_t on) {
  tsm::trace_launches(on != 0);
  return TSM_OK;
}

int64_t tsm_launch_trace(char *buf, int64_t cap) {
  const char *t = tsm::launch_trace();
  const int64_t need = (int64_t)strlen(t) + 1;
  if (buf && cap >= need) memcpy(buf, t, (size_t)need);
  return need;
}

const char *tsm_last_error(const tsm_engine *e) { return e ? e->err.c_str() : g_create_error.c_str(); }

int tsm_create(const tsm_config *cfg, tsm_engine **out) {
  if (!cfg || !out) return fail(nullptr, TSM_ERR_INVALID_ARG, "cfg/out is NULL");
  *out = nullptr;
  if (cfg->struct_size != (int32_t)sizeof(tsm_config))
    return fail(nullptr, TSM_ERR_INVALID_ARG, "tsm_config.struct_size mismatch (ABI)");
  if (cfg->num_class <= 0 || cfg->num_segments <= 0 || cfg->max_clips <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "num_class, num_segments, max_clips must be positive");
  if (cfg->height < 32 || cfg->width < 32)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "height/width must be >= 32");
  {  // the conv kernels index output rows (frames x stem output pixels) with 32-bit ints
    const int64_t rows = (int64_t)cfg->max_clips * cfg->num_segments * ((cfg->height + 1) / 2) * ((cfg->width + 1) / 2);
    if (rows >= (int64_t)1 << 31)
      return fail(nullptr, TSM_ERR_CAPACITY, "max_clips * num_segments * (H/2) * (W/2) must stay below 2^31");
  }
  if (const char *why = shift_div_refusal(cfg->shift_div, tsm::kPrecF32)) return fail(nullptr, TSM_ERR_UNSUPPORTED, why);
  if (prec_of_dtype(cfg->dtype) < 0)
    return fail(nullptr, TSM_ERR_UNSUPPORTED, "dtype must be TSM_DTYPE_F32, TSM_DTYPE_BF16X3 or TSM_DTYPE_BF16");
  if (const char *why = shift_div_refusal(cfg->shift_div, prec_of_dtype(cfg->dtype))) return fail(nullptr, TSM_ERR_UNSUPPORTED, why);
  int ndev = 0;
  hipError_t st = hipGetDeviceCount(&ndev);
  if (st != hipSuccess || ndev <= 0)
    return fail(nullptr, TSM_ERR_HIP, std::string("no HIP device: ") + hipGetErrorString(st));
  if (cfg->device_id < 0 || cfg->device_id >= ndev) return fail(nullptr, TSM_ERR_INVALID_ARG, "bad device_id");
  tsm_engine *e = new tsm_engine();
  e->cfg = *cfg;
  e->prec = prec_of_dtype(cfg->dtype);
  const auto on = [](const char *s) { return atoi(s) != 0; };
  env_read("TSM_AUTOTUNE", &e->autotune, on);
  env_read("TSM_STEM_DIRECT", &e->stem_direct, on);
  env_read("TSM_STEM_POOL", &e->stem_pool, on);
  env_read("TSM_STEM_PLANAR", &e->stem_planar, on);
  env_read("TSM_CONV_TILE", &e->force_tile, tsm::conv_tile_from_name);
  env_read("TSM_CONV_CODE", &e->force_code, atoi);
  env_read("TSM_POS_MAJOR", &e->pos_major, on);
  env_read("TSM_POS_BALANCE", &e->pos_balance, on);
  env_read("TSM_TILE_64X128", &e->tile_64x128, on);
  env_read("TSM_FUSE_CONV23", &e->fuse23, on);
  env_read("TSM_FUSE_BLOCK", &e->fuse_block, on);
  env_read("TSM_FUSE_C3C1", &e->fuse31, on);
  env_read("TSM_FUSE_FRONT", &e->fuse_front, on);
  env_read("TSM_WALK", &e->walk, on);
  env_read("TSM_POISON", &e->poison, on);
  // TSM_TUNE_CACHE=<file> names the tune cache; unset: a per-user default ($XDG_CACHE_HOME or $HOME/.cache, then
  // tsm_hip/tune_cache.txt), so that the second process on a machine pays no tuning pass; "", "0" or "off" disables it.
  const char *tc = getenv("TSM_TUNE_CACHE");
  if (!tc) e->tune_path = default_tune_cache_path();
  else if (*tc && strcmp(tc, "0") != 0 && strcmp(tc, "off") != 0) e->tune_path = tc;
  build_topology(e);
  st = hipSetDevice(cfg->device_id);
  if (st == hipSuccess) st = hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking);
  if (st == hipSuccess) st = hipDeviceGetAttribute(&e->n_cu, hipDeviceAttributeMultiprocessorCount, cfg->device_id);
  if (st == hipSuccess) st = hipEventCreate(&e->ev0);
  if (st == hipSuccess) st = hipEventCreate(&e->ev1);
  if (st != hipSuccess) {
    g_create_error = std::string("engine init: ") + hipGetErrorString(st);
    delete e;
    return TSM_ERR_HIP;
  }
  if (!e->tune_path.empty()) {
    hipDeviceProp_t prop;
    // (the build id -- csrc/, per-file options AND the build's extra definitions -- : codes of another build of the library
    //  are still SAFE, every code is validated against its layer at launch, but they were timed on other kernels, so they
    //  are not reused; the same goes for everything else that changes the timings: CU count, fused forms, stem forms)
    e->tune_sig = "abi" + std::to_string(TSM_ABI_VERSION) + " build " TSM_BUILD_ID " " +
                  (hipGetDeviceProperties(&prop, cfg->device_id) == hipSuccess ? std::string(prop.gcnArchName) : "?") +
                  " cu" + std::to_string(e->n_cu) +
                  " T" + std::to_string(cfg->num_segments) + " " + std::to_string(cfg->height) + "x" +
                  std::to_string(cfg->width) + " dtype" + std::to_string(cfg->dtype) + " shift" +
                  std::to_string(cfg->is_shift ? cfg->shift_div : 0) + " fuse" + std::to_string(e->fuse23) + "/" + std::to_string(e->fuse_block) + "/" + std::to_string(e->fuse31) + "/" + std::to_string(e->fuse_front) +
                  " stem" + std::to_string(e->stem_direct ? 1 : 0) +
                  std::to_string(e->stem_pool ? 1 : 0) + std::to_string(e->stem_planar ? 1 : 0);
    e->tune_sig_base = e->tune_sig.size();   // (retag_tune_sig appends the backbone and the placement)
  }
  *out = e;
  return TSM_OK;
}

int tsm_set_backbone(tsm_engine *e, int32_t depth) {
  if (int rc = check_before_weights(e, "tsm_set_backbone")) return rc;
  if (int rc = refuse_on_convnext(e, "tsm_set_backbone")) return rc;
  if (!find_backbone(depth)) return fail(e, TSM_ERR_UNSUPPORTED, "depth must be 18, 34 or 50");
  if (find_backbone(depth)->basic && e->width != 64)
    return fail(e, TSM_ERR_UNSUPPORTED, "a BasicBlock backbone (depth 18 / 34) has no bottleneck width: the engine's is " +
                                            std::to_string(e->width));
  if (find_backbone(depth)->basic && e->non_local)
    return fail(e, TSM_ERR_UNSUPPORTED, "non-local blocks need a Bottleneck backbone (depth 50)");
  e->depth = depth;
  e->backbone_set = 1;
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_bottleneck_width(tsm_engine *e, int32_t width_per_group) {
  if (int rc = check_before_weights(e, "tsm_set_bottleneck_width")) return rc;
  if (int rc = refuse_on_convnext(e, "tsm_set_bottleneck_width")) return rc;
  if (width_per_group != 64 && width_per_group != 128)
    return fail(e, TSM_ERR_UNSUPPORTED, "width_per_group must be 64 or 128 (wide_resnet50_2)");
  if (width_per_group != 64 && find_backbone(e->depth)->basic)
    return fail(e, TSM_ERR_UNSUPPORTED, "width_per_group 128 needs a Bottleneck backbone (depth 50): torchvision's BasicBlock "
                                        "supports 64 only");
  e->width = width_per_group;
  e->backbone_set = 1;
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_shift_place(tsm_engine *e, int32_t place) {
  if (int rc = check_before_weights(e, "tsm_set_shift_place")) return rc;
  if (int rc = refuse_on_convnext(e, "tsm_set_shift_place")) return rc;
  if (const char *why = shift_place_refusal(place, e->cfg.is_shift, e->cfg.shift_div)) return fail(e, TSM_ERR_UNSUPPORTED, why);
  e->place = place;
  e->backbone_set = 1;
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_non_local(tsm_engine *e, int32_t on) {
  if (int rc = check_before_weights(e, "tsm_set_non_local")) return rc;
  if (int rc = refuse_on_convnext(e, "tsm_set_non_local")) return rc;
  if (on != 0 && on != 1) return fail(e, TSM_ERR_UNSUPPORTED, "non_local must be 0 or 1");
  if (on && e->prec != tsm::kPrecF32)
    return fail(e, TSM_ERR_UNSUPPORTED, "non-local blocks run in TSM_DTYPE_F32 only (the bf16 formats' fused forms do not know the block)");
  if (on && find_backbone(e->depth)->basic)
    return fail(e, TSM_ERR_UNSUPPORTED, "non-local blocks need a Bottleneck backbone (depth 50)");
  if (on && e->temporal_pool) return fail(e, TSM_ERR_UNSUPPORTED, temporal_pool_refusal(e->prec, e->cfg.is_shift, e->cfg.num_segments, 1));
  e->non_local = on;
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_temporal_pool(tsm_engine *e, int32_t on) {
  if (int rc = check_before_weights(e, "tsm_set_temporal_pool")) return rc;
  if (int rc = refuse_on_convnext(e, "tsm_set_temporal_pool")) return rc;
  if (on != 0 && on != 1) return fail(e, TSM_ERR_UNSUPPORTED, "temporal_pool must be 0 or 1");
  if (on)
    if (const char *why = temporal_pool_refusal(e->prec, e->cfg.is_shift, e->cfg.num_segments, e->non_local)) return fail(e, TSM_ERR_UNSUPPORTED, why);
  e->temporal_pool = on;
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_convnext(tsm_engine *e, const int32_t depths[4]) {
  if (int rc = check_before_weights(e, "tsm_set_convnext")) return rc;
  if (!depths) return fail(e, TSM_ERR_INVALID_ARG, "tsm_set_convnext: depths is NULL");
  if (e->tdn) return fail(e, TSM_ERR_UNSUPPORTED, "tsm_set_convnext: a TDN engine (tsm_set_tdn) has no such part");
  if (const char *why = cnx_refusal(e->prec, e->cfg.is_shift, e->cfg.num_segments, e->backbone_set, e->non_local, e->temporal_pool, depths))
    return fail(e, TSM_ERR_UNSUPPORTED, std::string("tsm_set_convnext: ") + why);
  e->convnext = 1;
  for (int s = 0; s < kCnxStages; ++s) e->cnx_depths[s] = depths[s];
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_tdn(tsm_engine *e, const int32_t depths[4], float alpha, float beta) {
  if (int rc = check_before_weights(e, "tsm_set_tdn")) return rc;
  if (!depths) return fail(e, TSM_ERR_INVALID_ARG, "tsm_set_tdn: depths is NULL");
  if (!std::isfinite(alpha) || !std::isfinite(beta)) return fail(e, TSM_ERR_INVALID_ARG, "tsm_set_tdn: alpha and beta must be finite");
  const int other = e->convnext || e->backbone_set || e->non_local || e->temporal_pool;
  if (const char *why = tdn_refusal(e->prec, e->cfg.is_shift, e->cfg.num_segments, e->cfg.height, e->cfg.width, other, depths))
    return fail(e, TSM_ERR_UNSUPPORTED, std::string("tsm_set_tdn: ") + why);
  e->tdn = 1;
  e->tdn_alpha = alpha;
  e->tdn_beta = beta;
  for (int s = 0; s < 4; ++s) e->tdn_depths[s] = depths[s];
  build_topology(e);
  retag_tune_sig(e);
  return TSM_OK;
}

int tsm_set_consensus(tsm_engine *e, int32_t consensus) {
  if (int rc = check_before_weights(e, "tsm_set_consensus")) return rc;
  if (consensus != 0 && consensus != 1) return fail(e, TSM_ERR_UNSUPPORTED, "consensus must be 0 (avg) or 1 (identity)");
  e->consensus = consensus;   // (the head is not tuned: the tune signature does not carry it)
  return TSM_OK;
}

void tsm_destroy(tsm_engine *e) {
  if (!e) return;
  (void)hipSetDevice(e->cfg.device_id);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (void *p : e->allocs) (void)hipFree(p);
  for (auto &v : e->timing)
    for (hipEvent_t ev : v)
      if (ev) (void)hipEventDestroy(ev);
  for (hipEvent_t ev : e->event_pool) (void)hipEventDestroy(ev);
  if (e->ev0) (void)hipEventDestroy(e->ev0);
  if (e->ev1) (void)hipEventDestroy(e->ev1);
  if (e->stream) (void)hipStreamDestroy(e->stream);
  delete e;
}

int tsm_set_tensor(tsm_engine *e, const char *name, const float *host_data, const int64_t *shape,
                   int32_t ndim) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (!name || !host_data || !shape || ndim < 1 || ndim > 5) return fail(e, TSM_ERR_INVALID_ARG, "bad tensor args");   // (5: the non-local block's conv3d weights)
  if (e->finalized) return fail(e, TSM_ERR_INVALID_ARG, "engine already finalized");
  const std::string key(name);
  e->weights_started = true;
  if (!known_name(e, key)) return fail(e, TSM_ERR_INVALID_ARG, "unknown tensor name: " + key);
  HostTensor t;
  size_t elems = 1;
  for (int i = 0; i < ndim; ++i) {
    if (shape[i] <= 0) return fail(e, TSM_ERR_SHAPE, "non-positive dim in " + key);
    t.shape.push_back(shape[i]);
    elems *= (size_t)shape[i];
  }
  t.data.assign(host_data, host_data + elems);
  e->tensors[key] = std::move(t);
  return TSM_OK;
}

int tsm_finalize(tsm_engine *e) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (e->finalized) return TSM_OK;
  TSM_HIP(e, hipSetDevice(e->cfg.device_id));
  if (int rc = check_tensors(e)) return rc;
  const tsm_config &cfg = e->cfg;
  WeightAlloc alloc{e};
  // Every conv packed by its kind; the folded fp32 copies of a Bottleneck's 1x1 layers are kept for the fusions behind them.
  std::vector<std::vector<float>> host_wp(e->convs.size()), host_bias(e->convs.size());
  for (size_t ci = 0; ci < e->convs.size(); ++ci) {
    ConvLayer &c = e->convs[ci];
    std::vector<float> wp, bias;
    pack_conv(e, c, &wp, &bias);
    if (c.k == 1 && (c.kind == ConvKind::kBn || c.kind == ConvKind::kTdnBias)) {
      host_wp[ci] = wp;
      host_bias[ci] = bias;
    }
    if (int rc = upload_conv(e, alloc, e->prec, c.cout, &wp, bias, &c.d_w, &c.d_b)) return rc;
  }
  if (int rc = upload_block_fusions(e, alloc, host_wp, host_bias)) return rc;   // (a ConvNeXt engine has no blocks)
  host_wp.clear();
  host_bias.clear();
  if (e->convnext)
    if (int rc = upload_convnext_norms_and_dw(e, alloc)) return rc;
  if (int rc = upload_tdn_mse(e, alloc)) return rc;
  if (int rc = upload_pair(e, alloc, head_prefix(e), &e->d_fcw, &e->d_fcb, "d_fcw", "d_fcb")) return rc;

  // The workspace, sized per frame; both capacity refusals come before its first allocation.
  const int H = cfg.height, W = cfg.width;
  Workspace ws;
  ws.frames = (size_t)cfg.max_clips * cfg.num_segments;
  ws.in_frame = (size_t)(e->tdn ? kTdnPlanes : 3) * H * W;
  ws.in4_frame = (size_t)4 * H * (e->tdn ? W : W + 1);   // 16 bytes per pixel in every format (pairs: odd widths padded)
  if (e->convnext) {   // (num_segments is 1) the largest activation of the schedule is fc1's output in stage 0
    if (cnx_workspace_elems((int64_t)ws.frames, H, W) < 0)
      return fail(e, TSM_ERR_CAPACITY, "max_clips * (H / 4) * (W / 4) * 512 activations must stay below 2^29 (32-bit byte offsets)");
    ws.per_frame = (size_t)cnx_frame_elems(H, W);
    return alloc_workspace(e, ws);
  }
  e->h1 = conv_out_size(H, 7, 2);
  e->w1 = conv_out_size(W, 7, 2);
  e->hp = conv_out_size(e->h1, 3, 2);   // (the max-pool)
  e->wp = conv_out_size(e->w1, 3, 2);
  if (!e->tdn) {
    ws.per_frame = activation_frame_elems(e, (size_t)e->h1 * e->w1 * 64, &ws.mse_frame);
    return alloc_workspace(e, ws);
  }
  e->hd = tdn_diff_size(H);
  e->wd = tdn_diff_size(W);
  e->tdn_chunk = tdn_chunk_clips(cfg.max_clips, cfg.num_segments, H, W);
  if (e->tdn_chunk <= 0) return fail(e, TSM_ERR_CAPACITY, "the patch rows of conv1_5 for one clip, T * (H / 4) * (W / 4) * 1024 floats, must stay below 2^29");
  // (x_c5 and layer1's 256 channels on the stem's pooled map; the patch rows have their own buffer)
  ws.per_frame = activation_frame_elems(e, (size_t)e->hp * e->wp * 256, &ws.mse_frame);
  if ((double)ws.frames * (double)ws.per_frame >= (double)(kInt31 >> 2))
    return fail(e, TSM_ERR_CAPACITY, "max_clips * num_segments * (H / 4) * (W / 4) * 256 activations must stay below 2^29 (32-bit byte offsets)");
  ws.patch_frame = (size_t)tdn_conv15_size(H) * tdn_conv15_size(W) * kTdnPatchK;
  ws.patch_frames = (size_t)e->tdn_chunk * cfg.num_segments;
  return alloc_workspace(e, ws);
}

// tsm_forward (features = 0: `out` = the logits) and tsm_forward_features (1 / 2: `out` = the pooled / unit rows): one contract,
// one body.  The host-memory staging buffer of the output is d_logits or d_pooled, each sized for max_clips.
static int forward_to(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips, float *out,
                      int features, void *stream) {
  int rc = check_forward_args(e, clips, memkind, layout, n_clips);
  if (rc) return rc;
  if (layout == TSM_LAYOUT_TDN_SEGMENTS) {   // the segment phase has no head: its outputs are the descriptor's, `out` is ignored
    if (features) return fail(e, TSM_ERR_UNSUPPORTED, "tsm_forward_features: TSM_LAYOUT_TDN_SEGMENTS has no feature rows (the trunk phase has)");
  } else if (!out) {
    return fail(e, TSM_ERR_INVALID_ARG, features ? "features is NULL" : "logits is NULL");
  }
  hipStream_t s;
  const float *d_clips;
  if ((rc = stage_input(e, clips, memkind, layout, n_clips, stream, &s, &d_clips))) return rc;
  float *d_stage = features ? e->d_pooled : e->d_logits, *d_out = memkind == TSM_MEM_HOST ? d_stage : out;
  struct Mode {   // run_forward's last launch, for this call only (every return path)
    tsm_engine *e;
    ~Mode() { e->features = 0; }
  } mode{e};
  e->features = features;
  e->cur_timing = nullptr;
  if (e->timing_left > 0) {
    --e->timing_left;
    e->timing.emplace_back();
    e->cur_timing = &e->timing.back();
  }
  // A forward that still has to tune its tile shapes does so in a throw-away pass first (it uses the
  // timing events and synchronises); the real pass below then runs from the cache.
  rc = ensure_tuned(e, d_clips, layout, n_clips, d_out, s);
  if (rc) return rc;
  rc = poison_workspace(e, s);   // (TSM_POISON=1 only; after the tuning pass, before the forward proper)
  if (rc) return rc;
  TSM_HIP(e, hipEventRecord(e->ev0, s));
  rc = run_forward(e, d_clips, layout, n_clips, d_out, s, nullptr, nullptr);
  e->cur_timing = nullptr;
  if (rc) return rc;
  TSM_HIP(e, hipEventRecord(e->ev1, s));
  e->have_time = true;
  if (memkind == TSM_MEM_HOST) {
    const size_t elems = features ? (size_t)n_clips * out_segments(e) * e->feat
                                  : (size_t)n_clips * (e->consensus == 1 ? out_segments(e) : 1) * e->cfg.num_class;
    TSM_HIP(e, hipMemcpyAsync(out, d_stage, elems * sizeof(float), hipMemcpyDeviceToHost, s));
    TSM_HIP(e, hipStreamSynchronize(s));
  }
  return e->poison ? verify_guards(e, s) : TSM_OK;
}

int tsm_forward(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips,
                float *logits, void *stream) {
  return forward_to(e, clips, memkind, layout, n_clips, logits, 0, stream);
}

int tsm_forward_features(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips, float *features,
                         int32_t normalize, void *stream) {
  return forward_to(e, clips, memkind, layout, n_clips, features, normalize ? 2 : 1, stream);
}

int tsm_tune(tsm_engine *e, int32_t n_clips, void *stream) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (!e->finalized) return fail(e, TSM_ERR_NOT_FINALIZED, "tsm_finalize has not been called");
  if (n_clips <= 0) return fail(e, TSM_ERR_INVALID_ARG, "n_clips must be positive");
  if (n_clips > e->cfg.max_clips)
    return fail(e, TSM_ERR_CAPACITY, "n_clips " + std::to_string(n_clips) + " exceeds max_clips " + std::to_string(e->cfg.max_clips));
  const int tune_key = tile_bucket(n_clips) * e->cfg.num_segments;
  if (!e->autotune || e->tile_cache.find(tune_key) != e->tile_cache.end()) return TSM_OK;
  TSM_HIP(e, hipSetDevice(e->cfg.device_id));
  hipStream_t s = static_cast<hipStream_t>(stream);
  // the engine's own packed-input buffer, zeroed, stands in for a batch: no caller memory, no host copy, no kernel of
  // anybody else's (a cold process pays first-use code-object loads for those)
  const size_t frames = (size_t)n_clips * e->cfg.num_segments;
  if (e->tdn) {   // a TDN engine's input is the 15-plane tensor: its own staging buffer, zeroed, stands in (the front end fills d_in4)
    TSM_HIP(e, hipMemsetAsync(e->d_in, 0, frames * kTdnPlanes * e->cfg.height * e->cfg.width * sizeof(float), s));
    bool cached = false;
    int rct = ensure_tuned(e, e->d_in, TSM_LAYOUT_NTCHW, n_clips, e->d_logits, s, &cached);
    if (rct || !cached) return rct;
    std::vector<hipEvent_t> *keep = e->cur_timing;   // (as below: the bucket's forward once, so that every kernel is loaded)
    e->cur_timing = nullptr;
    rct = run_forward(e, e->d_in, TSM_LAYOUT_NTCHW, n_clips, e->d_logits, s, nullptr, nullptr);
    e->cur_timing = keep;
    return rct;
  }
  TSM_HIP(e, hipMemsetAsync(e->d_in4, 0, frames * 4 * e->cfg.height * (e->cfg.width + 1) * sizeof(float), s));
  const int layout = packed_layout_of(e->prec);
  bool from_file = false;
  int rc = ensure_tuned(e, e->d_in4, layout, n_clips, e->d_logits, s, &from_file);
  if (rc || !from_file) return rc;
  // The choices came from the cache file, so nothing has been launched yet: run the bucket's forward once on the zeroed
  // buffer anyway.  Every kernel of the schedule is then loaded (the library bundles one code object per kernel family,
  // each loaded lazily at its first launch) and the header's promise holds on this path too -- after tsm_tune a
  // tsm_forward of the bucket allocates nothing, loads nothing and synchronises nothing.
  std::vector<hipEvent_t> *saved = e->cur_timing;
  e->cur_timing = nullptr;
  rc = run_forward(e, e->d_in4, layout, n_clips, e->d_logits, s, nullptr, nullptr);
  e->cur_timing = saved;
  return rc;
}

int tsm_forward_tap(tsm_engine *e, const void *clips, int32_t memkind, int32_t layout, int32_t n_clips,
                    const char *stage, float *out, int64_t out_capacity, int64_t out_shape[4],
                    void *stream) {
  int rc = check_forward_args(e, clips, memkind, layout, n_clips);
  if (rc) return rc;
  if (!stage || !out || !out_shape) return fail(e, TSM_ERR_INVALID_ARG, "stage/out/out_shape is NULL");
  if (layout == TSM_LAYOUT_TDN_SEGMENTS || layout == TSM_LAYOUT_TDN_RING) {   // a stage on the other side of the seam: refused before any launch
    const bool front = tdn_stage_in_segment_phase(stage);
    if (front != (layout == TSM_LAYOUT_TDN_SEGMENTS))
      return fail(e, TSM_ERR_INVALID_ARG, std::string(front ? "the trunk phase starts at fuse2: no stage " : "the segment phase ends with layer1: no stage ") + stage);
  }
  hipStream_t s;
  const float *d_clips;
  if ((rc = stage_input(e, clips, memkind, layout, n_clips, stream, &s, &d_clips))) return rc;
  rc = poison_workspace(e, s);
  if (rc) return rc;
  Tap tap;
  rc = run_forward(e, d_clips, layout, n_clips, e->d_logits, s, stage, &tap);
  if (rc) return rc;
  const int64_t elems = tap.shape[0] * tap.shape[1] * tap.shape[2] * tap.shape[3];
  for (int i = 0; i < 4; ++i) out_shape[i] = tap.shape[i];
  if (elems > out_capacity) return fail(e, TSM_ERR_CAPACITY, "tap output buffer too small");
  if (e->prec != tsm::kPrecF32) {  // taps are reported as fp32 whatever the storage format
    if (!e->d_tap) {
      const size_t cap = std::max(e->buf_elems, (size_t)e->cfg.max_clips * e->cfg.num_segments * 8 * e->cfg.height * e->cfg.width);
      rc = dev_alloc(e, &e->d_tap, cap, "d_tap", cap / ((size_t)e->cfg.max_clips * e->cfg.num_segments));
      if (rc) return rc;
    }
    TSM_HIP(e, tsm::launch_to_f32(tap.ptr, e->d_tap, elems / 8, e->prec, s));
    tap.ptr = e->d_tap;
  }
  TSM_HIP(e, hipMemcpyAsync(out, tap.ptr, (size_t)elems * sizeof(float),
                            memkind == TSM_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice, s));
  TSM_HIP(e, hipStreamSynchronize(s));
  return e->poison ? verify_guards(e, s) : TSM_OK;
}

int tsm_set_layer_timing(tsm_engine *e, int32_t n_forwards, int32_t only_conv3x3) {
  if (!e) return TSM_ERR_INVALID_ARG;
  if (n_forwards < 0 || n_forwards > 64) return fail(e, TSM_ERR_INVALID_ARG, "n_forwards must be in [0, 64]");
  e->timing_only3x3 = only_conv3x3 != 0;
  for (auto &v : e->timing)
    for (hipEvent_t ev : v)
      if (ev) e->event_pool.push_back(ev);
  e->timing.clear();
  e->timing.reserve(64);
  e->timing_left = n_forwards;
  return TSM_OK;
}

int tsm_layer_times(tsm_engine *e, int32_t forward_index, float *ms_out, int32_t cap, int32_t *n_out) {
  if (!e || !ms_out || !n_out) return TSM_ERR_INVALID_ARG;
  if (forward_index < 0 || forward_index >= (int32_t)e->timing.size())
    return fail(e, TSM_ERR_INVALID_ARG, "no timing recorded for that forward");
  const std::vector<hipEvent_t> &ev = e->timing[forward_index];
  const int n = (int)ev.size() / 2;
  *n_out = n;
  if (n > cap) return fail(e, TSM_ERR_CAPACITY, "ms_out too small");
  for (int i = 0; i < n; ++i) {
    ms_out[i] = -1.f;
    if (!ev[2 * i] || !ev[2 * i + 1]) continue;
    TSM_HIP(e, hipEventSynchronize(ev[2 * i + 1]));
    TSM_HIP(e, hipEventElapsedTime(&ms_out[i], ev[2 * i], ev[2 * i + 1]));
  }
  return TSM_OK;
}

int tsm_conv_tiles(tsm_engine *e, int32_t n_clips, int32_t *tiles_out, int32_t cap, int32_t *n_out) {
  if (!e || !tiles_out || !n_out) return TSM_ERR_INVALID_ARG;
  // Report what RUNS: a fusion bit only where an n_clips forward runs that form (its plan), whatever a hand-edited or
  // bucket-shared code says; a form forced through TSM_FUSE_* = 1 is not a tuner choice and carries no bit.
  std::vector<int> codes(e->convs.size(), 0);
  auto it = e->tile_cache.find(tile_bucket(n_clips) * e->cfg.num_segments);
  if (it != e->tile_cache.end()) {
    const std::vector<BlockPlan> plan = plan_forward(e, &it->second, n_clips * e->cfg.num_segments, nullptr);
    for (size_t i = 0; i < codes.size(); ++i) codes[i] = it->second[i] & ~kCodeFused;
    for (size_t k = 0; k < e->blocks.size(); ++k) {
      const Block &b = e->blocks[k];
      const BlockPlan &p = plan[k];
      codes[b.conv1] |= it->second[b.conv1] & ((p.block ? kCodeBlock : 0) | (p.front ? kCodeFront : 0));
      if (p.conv23) codes[b.conv2] |= it->second[b.conv2] & kCodeConv23;
      if (p.conv31_next) codes[b.conv3] |= it->second[b.conv3] & kCodeConv31;
    }
  }
  // launch order: stem, then per block [downsample,] conv1, conv2, conv3 (Bottleneck) / [downsample,] conv1, conv2 (BasicBlock)
  // [, the wrapper's theta | phi | g and W convs]
  std::vector<int> order{0};
  if (e->tdn) order.push_back(1);   // (a TDN engine: the stem, conv1_5, then resnext_layer1's and the trunk's blocks)
  for (const Block &b : e->blocks)
    for (int ci : {b.down, b.conv1, b.conv2, b.conv3, b.nl_qkv, b.nl_w})
      if (ci >= 0) order.push_back(ci);
  for (size_t ci = 1; e->convnext && ci < e->convs.size(); ++ci) order.push_back((int)ci);   // (a ConvNeXt engine's convs are in launch order)
  *n_out = (int32_t)order.size();
  if ((int)order.size() > cap) return fail(e, TSM_ERR_CAPACITY, "tiles_out too small");
  for (size_t i = 0; i < order.size(); ++i) tiles_out[i] = codes[order[i]];
  return TSM_OK;
}

float tsm_last_forward_ms(tsm_engine *e) {
  if (!e || !e->have_time) return -1.f;
  if (hipEventSynchronize(e->ev1) != hipSuccess) return -1.f;
  float ms = -1.f;
  if (hipEventElapsedTime(&ms, e->ev0, e->ev1) != hipSuccess) return -1.f;
  return ms;
}

// ---- per-op entry points (device pointers) ----------------------------------------------------

int tsm_temporal_shift(const float *x, float *y, int64_t n_frames, int32_t n_segment, int64_t hw, int32_t c,
                       int32_t fold_div, void *stream) {
  if (!x || !y || n_frames <= 0 || hw <= 0 || c <= 0 || fold_div <= 0) return TSM_ERR_INVALID_ARG;
  const int fold = c / fold_div;
  return op_status("temporal_shift", tsm::launch_temporal_shift(x, y, n_frames, n_segment, hw, c, fold, static_cast<hipStream_t>(stream)));
}

int tsm_conv_op(const tsm_conv_args *a, void *stream) {
  const ConvOpPlan pl = conv_op_check(a);   // every refusal, before the first HIP call
  if (pl.status != TSM_OK) return fail(nullptr, pl.status, pl.message);
  const int prec = pl.prec, n = a->n, hi = a->hi, wi = a->wi, cout = a->cout;
  const bool x3 = prec != tsm::kPrecF32;  // any non-fp32 storage format: convert at the boundary
  hipStream_t s = static_cast<hipStream_t>(stream);
  TSM_HIP(nullptr, hipStreamSynchronize(s));
  // The weights, prepared as tsm_finalize prepares a layer's (a second source: as its conv3 + downsample GEMM's).
  ConvLayer c, c2;
  static_cast<LayerGeom &>(c) = pl.geo;
  c.kseg = pl.kseg;   // (a single source runs whole-K here unless the code asks for the engine's segments: kCodeOpSegmented)
  c.cin = a->cin; c.cout = cout; c.k = a->k; c.stride = a->stride;
  std::vector<float> wp, bias;
  if (int rc = fetch_prepared(c, a->w, a->gamma, a->beta, a->mean, a->var, &wp, &bias)) return rc;
  if (pl.dual) {
    std::vector<float> wp2, bias2, wf, bf;
    c2.cin = c2.cp = a->cin2; c2.cout = cout; c2.kp = pl.kp2;
    if (int rc = fetch_prepared(c2, a->w2, a->gamma2, a->beta2, a->mean2, a->var2, &wp2, &bias2)) return rc;
    concat_k_pair(wp, bias, c.kp, wp2, bias2, c2.kp, cout, &wf, &bf);
    wp.swap(wf);
    bias.swap(bf);
  }
  GuardedScratch scratch;
  auto alloc = [&scratch](float **q, const char *name, size_t elems, size_t frame_elems) { return scratch.alloc(q, name, elems, frame_elems); };
  int rc = upload_conv(nullptr, alloc, prec, cout, &wp, bias, &c.d_w, &c.d_b);
  if (rc) return rc;
  // The operands in the storage format (fp32: the caller's own, but for the stem's NHWC3 -> NHWC4 / pixel pairs).
  const size_t act_bytes = prec == tsm::kPrecBf16 ? 2 : 4;   // bytes per stored activation element (split-bf16: hi + lo = 4)
  const size_t in_px = (size_t)hi * wi, out_frame = (size_t)pl.ho * pl.wo * cout, out_elems = (size_t)pl.y_elems;
  auto staged = [&](const float *src, const char *name, size_t elems, size_t frame_elems, const float **dst) -> int {
    float *d = nullptr;
    if (int r = scratch.alloc(&d, name, elems, frame_elems, act_bytes)) return r;
    TSM_HIP(nullptr, tsm::launch_from_f32(src, d, (int64_t)elems / 8, prec, s));
    *dst = d;
    return TSM_OK;
  };
  const float *xin = a->x, *x2in = a->x2, *rin = a->residual;
  float *yout = a->y, *d_x4 = nullptr, *d_ys = nullptr, *d_part = nullptr;
  if (pl.stem) {
    if ((rc = scratch.alloc(&d_x4, "d_x4", n * in_px * 8, in_px * 8))) return rc;
    TSM_HIP(nullptr, tsm::launch_pack_input(a->x, d_x4, n, hi, wi, 0, prec, s));
    xin = d_x4;
  } else if (x3 && (rc = staged(a->x, "d_xs", (size_t)pl.x_elems, in_px * a->cin, &xin))) {
    return rc;
  }
  if (x3) {
    if ((rc = scratch.alloc(&d_ys, "d_ys", out_elems, out_frame, act_bytes))) return rc;
    yout = d_ys;
    if (rin && (rc = staged(rin, "d_rs", out_elems, out_frame, &rin))) return rc;
    if (pl.dual && (rc = staged(x2in, "d_x2s", (size_t)pl.x2_elems, (size_t)a->hi2 * a->wi2 * a->cin2, &x2in))) return rc;
  }
  tsm::ConvParams p = make_params(c, xin, rin, yout, n, hi, wi, a->relu != 0, pl.T, 1, prec);
  p.fold = pl.fold;
  p.reverse = a->reverse != 0;
  if (pl.dual) set_second_source(&p, c2.kp, x2in, a->cin2, a->hi2, a->wi2, a->stride2);
  int dev = 0, n_cu = 256;
  TSM_HIP(nullptr, hipGetDevice(&dev));
  TSM_HIP(nullptr, hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev));
  // the code as Forward::conv takes it; the split forms get a segment scratch of their own
  const int code = checked_code(p, a->code > 0 ? a->code & ~kCodeOpSegmented : a->code, n_cu);
  size_t part_elems = 0;
  if ((code & (kCodeSplitK | kCodeTailK)) && p.kseg_len > 0) {
    part_elems = (size_t)tsm::conv_num_segments(p) * p.M * p.Cout;
    if ((rc = scratch.alloc(&d_part, "d_part", part_elems, out_frame))) return rc;
  }
  // (a test / debug entry point that packs weights and allocates on every call: its tuning hook is read per call)
  const char *sd_env = getenv("TSM_STEM_DIRECT"), *pb_env = getenv("TSM_POS_BALANCE");
  hipError_t st;
  if (pl.stem && x3 && cout == 64 && !(sd_env && atoi(sd_env) == 0))
    st = tsm::launch_stem_direct(xin, c.d_w, c.d_b, yout, n, hi, wi, c.kp, a->relu != 0, prec, s);
  else
    st = launch_conv_code(p, a->k, code, d_part, part_elems, n_cu, s, !(pb_env && atoi(pb_env) == 0));
  if (st == hipSuccess && x3) st = tsm::launch_to_f32(d_ys, a->y, (int64_t)out_elems / 8, prec, s);
  const hipError_t st2 = hipStreamSynchronize(s);
  if (st != hipSuccess) return op_status("launch_conv", st);
  if (st2 != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("conv sync: ") + hipGetErrorString(st2));
  for (int i = 0; i < scratch.n; ++i) {
    std::string msg;
    TSM_HIP(nullptr, guard_verify(scratch.g[i], &msg));
    if (!msg.empty()) return fail(nullptr, TSM_ERR_GUARD, "tsm_conv_op: " + msg);
  }
  return TSM_OK;
}

int tsm_conv_bn_act(const float *x, const float *w, const float *gamma, const float *beta, const float *mean,
                    const float *var, const float *residual, float *y, int32_t n, int32_t hi, int32_t wi,
                    int32_t cin, int32_t cout, int32_t k, int32_t stride, int32_t relu, int32_t shift_segments,
                    int32_t fold_div, int32_t dtype, void *stream) {
  tsm_conv_args a{};
  a.struct_size = sizeof(tsm_conv_args);
  a.x = x; a.w = w; a.gamma = gamma; a.beta = beta; a.mean = mean; a.var = var; a.residual = residual; a.y = y;
  a.n = n; a.hi = hi; a.wi = wi; a.cin = cin; a.cout = cout; a.k = k; a.stride = stride; a.relu = relu;
  a.shift_segments = shift_segments; a.fold_div = fold_div; a.dtype = dtype;
  // (no engine, so the tuning hook is read per call: a tile TSM_CONV_TILE names, where it fits the launch)
  a.code = tsm::conv_tile_from_name(getenv("TSM_CONV_TILE"));
  return tsm_conv_op(&a, stream);
}

int tsm_maxpool3x3s2(const float *x, float *y, int32_t n, int32_t hi, int32_t wi, int32_t c, void *stream) {
  if (!x || !y || n <= 0 || hi <= 0 || wi <= 0) return TSM_ERR_INVALID_ARG;
  return op_status("maxpool", tsm::launch_maxpool3x3s2(x, y, n, hi, wi, c, tsm::kPrecF32, static_cast<hipStream_t>(stream)));
}

int tsm_maxpool2x2(const float *x, int64_t ld, int32_t c0, int32_t c, float *y, int32_t n, int32_t hi, int32_t wi, void *stream) {
  if (!x || !y || n <= 0 || c <= 0 || c0 < 0) return fail(nullptr, TSM_ERR_INVALID_ARG, "maxpool2x2: NULL pointer or non-positive size");
  if (hi < 2 || wi < 2) return fail(nullptr, TSM_ERR_INVALID_ARG, "maxpool2x2: needs at least 2 x 2 pixels");
  return op_status("maxpool2x2", tsm::launch_maxpool2x2(x, ld, c0, c, y, n, hi, wi, static_cast<hipStream_t>(stream)),
                   "c0, c and ld must be multiples of 4 with c0 + c <= ld, and the pointers 16-byte aligned");
}

int tsm_nonlocal_attention(const float *q, int64_t ldq, const float *k, const float *v, int64_t ldkv, float *y, int64_t ldy,
                           int32_t n_clips, int32_t nq, int32_t nk, int32_t d, void *stream) {
  if (d != 256 && d != 512) return fail(nullptr, TSM_ERR_UNSUPPORTED, "nonlocal_attention: d must be 256 or 512, got " + std::to_string(d));
  if (!q || !k || !v || !y || n_clips <= 0 || nq <= 0 || nk <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "nonlocal_attention: NULL pointer or non-positive size");
  return op_status("nonlocal_attention",
                   tsm::launch_nonlocal_attention(q, ldq, k, v, ldkv, y, ldy, n_clips, nq, nk, d, static_cast<hipStream_t>(stream)),
                   "row strides must be >= d (ldq, ldkv multiples of 4), q / k / v 16-byte aligned, n_clips <= 65535");
}

int tsm_preprocess(const void *frames, int32_t pixel, int32_t n, int32_t h, int32_t w, float *out,
                   int32_t out_layout, int32_t resize, int32_t crop, int32_t scale_255, void *stream) {
  if (!frames || !out || n <= 0 || h <= 0 || w <= 0 || resize <= 0 || crop <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "bad preprocess arguments");
  tsm::PreprocParams p{};
  if (int rc = set_pixel_format(&p, pixel, out_layout, scale_255)) return rc;
  if (int rc = check_yuv_frames("preprocess", pixel, frames, h, w)) return rc;
  p.src = frames; p.dst = out; p.n = n;
  if (!set_crop_geometry(&p, h, w, resize, crop)) return fail(nullptr, TSM_ERR_INVALID_ARG, "crop larger than the resized frame");
  return op_status("preprocess", tsm::launch_preprocess(p, static_cast<hipStream_t>(stream)));
}

int tsm_gather_clips(const void *frames, int64_t n_frames, int64_t frame_bytes, int64_t first_frame, int64_t total_frames,
                     int64_t pad_frame, int64_t first_clip, int32_t n_clips, int32_t n_segment, int32_t clip_step,
                     int32_t clip_stride, void *out, void *stream) {
  if (!frames || !out) return fail(nullptr, TSM_ERR_INVALID_ARG, "gather_clips: null pointer");
  tsm::GatherParams p{};
  p.frames = frames; p.out = out; p.n_frames = n_frames; p.frame_bytes = frame_bytes; p.first_frame = first_frame;
  p.total_frames = total_frames; p.first_clip = first_clip; p.pad_frame = pad_frame; p.n_clips = n_clips;
  p.n_segment = n_segment; p.clip_step = clip_step; p.clip_stride = clip_stride;
  return op_status("gather_clips", tsm::launch_gather_clips(p, static_cast<hipStream_t>(stream)),
                   "a clip of the range reads outside the frame buffer, the pad frame is one of the range's video frames, or frame_bytes is not a multiple of 16");
}

int tsm_preprocess_clips(const void *frames, int32_t pixel, int64_t n_frames, int32_t h, int32_t w, int64_t first_frame,
                         int64_t total_frames, int64_t first_clip, int32_t n_clips, int32_t n_segment, int32_t clip_step,
                         int32_t clip_stride, const int32_t *boxes, float *out, int32_t out_layout, int32_t size,
                         int32_t scale_255, void *stream) {
  if (!frames || !boxes || !out) return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_clips: null pointer");
  if (n_frames <= 0 || h <= 0 || w <= 0 || size <= 0 || n_clips <= 0 || n_segment <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_clips: non-positive size");
  tsm::ClipPreprocParams p{};
  if (int rc = set_pixel_format(&p, pixel, out_layout, scale_255)) return rc;
  if (int rc = check_yuv_frames("preprocess_clips", pixel, frames, h, w)) return rc;
  p.src = frames; p.dst = out; p.boxes = boxes; p.n_frames = n_frames; p.first_frame = first_frame;
  p.total_frames = total_frames; p.first_clip = first_clip; p.n_clips = n_clips; p.n_segment = n_segment;
  p.clip_step = clip_step; p.clip_stride = clip_stride; p.h = h; p.w = w; p.size = size;
  return op_status("preprocess_clips", tsm::launch_preprocess_clips(p, static_cast<hipStream_t>(stream)),
                   "clip_step is not a multiple of clip_stride, a clip starts past the end of the video, or a clip of the range reads outside the frame buffer");
}

int tsm_preprocess_indexed(const void *frames, int32_t pixel, int64_t n_frames, int32_t h, int32_t w, const int32_t *index,
                           int32_t n_clips, int32_t n_segment, float *out, int32_t out_layout, int32_t resize, int32_t crop,
                           int32_t scale_255, void *stream) {
  if (!frames || !index || !out) return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_indexed: null pointer");
  if (n_frames <= 0 || h <= 0 || w <= 0 || n_clips <= 0 || n_segment <= 0 || resize <= 0 || crop <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_indexed: non-positive size");
  tsm::IndexedPreprocParams q{};
  tsm::PreprocParams &p = q.pp;
  if (int rc = set_pixel_format(&p, pixel, out_layout, scale_255)) return rc;
  if (int rc = check_yuv_frames("preprocess_indexed", pixel, frames, h, w)) return rc;
  q.index = index; q.n_frames = n_frames; q.n_rows = (int64_t)n_clips * n_segment;
  p.src = frames; p.dst = out;
  if (!set_crop_geometry(&p, h, w, resize, crop))
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_indexed: crop larger than the resized frame");
  return op_status("preprocess_indexed", tsm::launch_preprocess_indexed(q, static_cast<hipStream_t>(stream)));
}

int tsm_preprocess_windows(const void *arena, int64_t arena_bytes, int32_t pixel, const int32_t *desc,
                           int32_t n_windows, int32_t n_segment, int32_t person_crop, float *out,
                           int32_t out_layout, int32_t resize, int32_t crop, int32_t scale_255, void *stream) {
  if (!arena || !desc || !out) return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: null pointer");
  if ((reinterpret_cast<uintptr_t>(arena) & 15) != 0 || (reinterpret_cast<uintptr_t>(desc) & 15) != 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: arena and desc must be 16-byte aligned");
  if (arena_bytes <= 0 || n_windows <= 0 || n_segment <= 0 || resize <= 0 || crop <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: non-positive size");
  tsm::WindowPreprocParams p{};
  if (int rc = set_pixel_format(&p, pixel, out_layout, scale_255)) return rc;
  if (person_crop == TSM_WINDOWS_IMAGE) {
    if (scale_255) return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: the image transform takes scale_255 = 0 (it divides by 255 itself)");
    if (crop > resize) return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: crop larger than the resized frame");
    if (pixel != TSM_PIXEL_U8 && !tsm_host::pixel_is_nv12(pixel))
      return fail(nullptr, TSM_ERR_UNSUPPORTED, "preprocess_windows: the image transform takes TSM_PIXEL_U8 or TSM_PIXEL_NV12_* frames");
    if (crop > tsm_host::kImageMaxCrop)
      return fail(nullptr, TSM_ERR_UNSUPPORTED, "preprocess_windows: one row of crop " + std::to_string(crop) + " does not fit 64 KB of LDS");
    p.arena = arena; p.dst = out; p.desc = desc; p.arena_bytes = arena_bytes; p.n_windows = n_windows; p.n_segment = n_segment;
    p.person_crop = person_crop; p.resize = resize; p.crop = crop;
    return op_status("preprocess_windows", tsm::launch_preprocess_image_windows(p, static_cast<hipStream_t>(stream)));
  }
  if (person_crop != 0 && person_crop != 1)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: person_crop must be 0, 1 or TSM_WINDOWS_IMAGE");
  if (!person_crop && crop > resize)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_windows: crop larger than the resized frame");
  p.arena = arena; p.dst = out; p.desc = desc; p.arena_bytes = arena_bytes; p.n_windows = n_windows; p.n_segment = n_segment;
  p.person_crop = person_crop; p.resize = resize; p.crop = crop;
  return op_status("preprocess_windows", tsm::launch_preprocess_windows(p, static_cast<hipStream_t>(stream)));
}

int tsm_top1_tally(const float *logits, const int32_t *labels, int32_t n, int32_t num_class, int32_t *pred, int32_t *correct,
                   int32_t *total, void *stream) {
  if (!logits || !labels || !correct || !total || n <= 0 || num_class <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "top1_tally: NULL pointer or non-positive size");
  if (correct == total) return fail(nullptr, TSM_ERR_INVALID_ARG, "top1_tally: correct and total must not alias");
  if (num_class > tsm::kTallyMaxClass)
    return fail(nullptr, TSM_ERR_UNSUPPORTED, "top1_tally: num_class must be at most " + std::to_string(tsm::kTallyMaxClass));
  hipError_t st = tsm::launch_top1_tally(logits, labels, n, num_class, pred, correct, total, static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("top1_tally: ") + hipGetErrorString(st));
  return TSM_OK;
}

// taps per row of Pillow's coefficient table for one axis (Resample.c precompute_coeffs: ksize = ceil(support) * 2 + 1)
static int pil_ksize(int in, int out) {
  const double scale = (double)in / out, support = scale < 1.0 ? 1.0 : scale;
  return (int)std::ceil(support) * 2 + 1;
}

int tsm_preprocess_image(const void *frames, int32_t n, int32_t h, int32_t w, const int32_t *tables, int64_t table_words,
                         float *out, int32_t out_layout, int32_t resize, int32_t crop, void *stream) {
  if (!frames || !out || n <= 0 || h <= 0 || w <= 0 || resize <= 0 || crop <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_image: NULL pointer or non-positive size");
  tsm::ImagePreprocParams p{};
  if (int rc = out_mode_of(out_layout, &p.out_mode)) return rc;
  p.src = static_cast<const unsigned char *>(frames); p.dst = out; p.n = n;
  if (!set_crop_geometry(&p, h, w, resize, crop))          // (torchvision's Resize(int) + center_crop on a PIL image: the same rule)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_image: crop larger than the resized frame");
  // the table block: [hb 2 * crop][hk crop * ksx] when the width changes, then [vb 2 * crop][vk crop * ksy] when the height does
  const bool horiz = p.nw != w, vert = p.nh != h;
  p.ksx = horiz ? pil_ksize(w, p.nw) : 0;
  p.ksy = vert ? pil_ksize(h, p.nh) : 0;
  const int64_t hwords = horiz ? (int64_t)crop * (2 + p.ksx) : 0, vwords = vert ? (int64_t)crop * (2 + p.ksy) : 0;
  if (table_words != hwords + vwords || (table_words > 0 && !tables))
    return fail(nullptr, TSM_ERR_INVALID_ARG, "preprocess_image: the table block must hold " + std::to_string(hwords + vwords) +
                " int32 words for this geometry (crop * (2 + taps) per resampled axis), got " + std::to_string(table_words));
  if (horiz) { p.hb = tables; p.hk = tables + 2 * (int64_t)crop; }
  if (vert) { p.vb = tables + hwords; p.vk = tables + hwords + 2 * (int64_t)crop; }
  hipError_t st = tsm::launch_preprocess_image(p, static_cast<hipStream_t>(stream));
  if (st == hipErrorNotSupported)
    return fail(nullptr, TSM_ERR_UNSUPPORTED, "preprocess_image: the rows under one output row's vertical support do not fit 64 KB "
                "of LDS (downscale " + std::to_string(h) + " -> " + std::to_string(p.nh) + " lines at crop " + std::to_string(crop) + ")");
  return op_status("preprocess_image", st);
}

int tsm_frame_votes(const float *logits, int32_t n_frames, int32_t num_class, const int32_t *history, int32_t n_hist,
                    int32_t *pred, int32_t *state, int32_t *history_out, void *stream) {
  if (!logits || !pred || !state || n_frames <= 0 || num_class <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "frame_votes: NULL pointer or non-positive size");
  if (n_hist < 0 || n_hist > 6 || (n_hist > 0 && !history))
    return fail(nullptr, TSM_ERR_INVALID_ARG, "frame_votes: n_hist must be 0..6, with a history of that many entries");
  if (history_out && history_out == history)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "frame_votes: history_out must not alias history");
  hipError_t st = tsm::launch_frame_votes(logits, n_frames, num_class, history, n_hist, pred, state, history_out,
                                          static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("frame_votes: ") + hipGetErrorString(st));
  return TSM_OK;
}

int tsm_head(const float *feat, const float *fc_w, const float *fc_b, float *logits, int32_t n_clips,
             int32_t n_segment, int32_t hw, int32_t c, int32_t num_class, void *stream) {
  if (!feat || !fc_w || !fc_b || !logits || n_clips <= 0 || n_segment <= 0 || hw <= 0 || c <= 0 || num_class <= 0)
    return TSM_ERR_INVALID_ARG;
  hipStream_t s = static_cast<hipStream_t>(stream);
  // The pooled rows between the two launches live in a stream-ordered allocation: allocated and freed ON `s`, so the call only
  // enqueues, and inside a stream capture the pair becomes the graph's own allocation and free nodes.
  float *pooled = nullptr;
  hipError_t st = hipMallocAsync(reinterpret_cast<void **>(&pooled), (size_t)n_clips * n_segment * c * sizeof(float), s);
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("head scratch: ") + hipGetErrorString(st));
  st = tsm::launch_head(feat, fc_w, fc_b, pooled, logits, n_clips, n_segment, hw, c, num_class, tsm::kPrecF32, s);
  const hipError_t st2 = hipFreeAsync(pooled, s);
  if (st != hipSuccess || st2 != hipSuccess)
    return fail(nullptr, TSM_ERR_HIP, std::string("head: ") + hipGetErrorString(st != hipSuccess ? st : st2));
  return TSM_OK;
}

int tsm_head_segments(const float *feat, const float *fc_w, const float *fc_b, float *logits, int32_t n_frames, int32_t hw,
                      int32_t c, int32_t num_class, void *stream) {
  if (!feat || !fc_w || !fc_b || !logits || n_frames <= 0 || hw <= 0 || c <= 0 || num_class <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "head_segments: NULL pointer or non-positive size");
  if (c % 8 != 0 || c > 2048) return fail(nullptr, TSM_ERR_UNSUPPORTED, "head_segments: c must be a multiple of 8, at most 2048");
  hipError_t st = tsm::launch_head_segments(feat, fc_w, fc_b, logits, n_frames, hw, c, num_class, tsm::kPrecF32,
                                            static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("head_segments: ") + hipGetErrorString(st));
  return TSM_OK;
}

int tsm_pool_features(const float *feat, float *pooled, float *unit, int32_t n_frames, int32_t hw, int32_t c, void *stream) {
  if (!feat || (!pooled && !unit) || n_frames <= 0 || hw <= 0 || c <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "pool_features: NULL pointer (feat, or both outputs) or non-positive size");
  if ((reinterpret_cast<uintptr_t>(feat) | reinterpret_cast<uintptr_t>(pooled) | reinterpret_cast<uintptr_t>(unit)) & 15u)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "pool_features: pointers must be 16-byte aligned");
  if (c % 8 != 0 || c > 2048) return fail(nullptr, TSM_ERR_UNSUPPORTED, "pool_features: c must be a multiple of 8, at most 2048");
  hipError_t st = tsm::launch_pool_features(feat, pooled, unit, n_frames, hw, c, tsm::kPrecF32, static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("pool_features: ") + hipGetErrorString(st));
  return TSM_OK;
}

int tsm_cosine_distances(const float *unit, int32_t n_total, int32_t c, int32_t row0, int32_t row1, float *dist, void *stream) {
  if (!unit || !dist) return fail(nullptr, TSM_ERR_INVALID_ARG, "cosine_distances: NULL pointer");
  if ((reinterpret_cast<uintptr_t>(unit) | reinterpret_cast<uintptr_t>(dist)) & 15u)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "cosine_distances: pointers must be 16-byte aligned");
  if (row0 < 0 || row0 >= row1 || row1 > n_total || c <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "cosine_distances: need 0 <= row0 < row1 <= n_total and c > 0");
  if (c % 8 != 0) return fail(nullptr, TSM_ERR_UNSUPPORTED, "cosine_distances: c must be a multiple of 8");
  hipError_t st = tsm::launch_cosine_distances(unit, n_total, c, row0, row1, dist, static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("cosine_distances: ") + hipGetErrorString(st));
  return TSM_OK;
}

int tsm_scores_to_states(const float *logits, int32_t n_clips, int32_t num_class, int32_t softmax, float threshold,
                         int32_t *states, float *top_score, void *stream) {
  if (!logits || !states || n_clips <= 0 || num_class <= 0)
    return fail(nullptr, TSM_ERR_INVALID_ARG, "scores_to_states: NULL pointer or non-positive size");
  hipError_t st = tsm::launch_scores_to_states(logits, n_clips, num_class, softmax != 0, threshold, states, top_score,
                                               static_cast<hipStream_t>(stream));
  if (st != hipSuccess) return fail(nullptr, TSM_ERR_HIP, std::string("scores_to_states: ") + hipGetErrorString(st));
  return TSM_OK;
}

}  // extern "C"
