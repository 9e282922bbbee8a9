// The conv launch rules, each stated once: the parameter blocks of the conv launchers, the LDS-budget constants and tile
// geometries of the weight-stationary kernels, every kernel family's "does it apply?" and grid rule, and conv_route(), which
// decides from shapes alone whether a launch_conv call is refused and which kernel family, template arm, tile counts, grid and
// geometry it runs with.  The launchers (csrc/tsm_*.hip) only launch what the route says.  No HIP types and no device query
// (the CU count is an argument), so this header also compiles with plain g++: tests/host_sanitize.cpp drives it under
// -fsanitize=address,undefined.  Pointers are compared with NULL (res, x2) and never read.
#pragma once
#include <stdint.h>
#include <string.h>

#if defined(__HIPCC__)
#define TSM_HOST_DEVICE __host__ __device__
#else
#define TSM_HOST_DEVICE
#endif

namespace tsm {

struct ConvParams {
  const float *x;     // [N, Hi, Wi, C]   C = 4 (stem, padded) or a multiple of 32
  const float *w;     // [Cout][Kp]       BN scale folded in, zero padded to Kp
  const float *bias;  // [Cout]           folded BN bias
  const float *res;   // nullable [M, Cout] residual added before the activation
  float *y;           // [M, Cout]
  int N, Hi, Wi, C, logC4;  // (C / 4) == 1 << logC4
  int Ho, Wo, Cout;
  int stride, pad;
  int Kp;    // padded K, multiple of 32
  int M;     // N * Ho * Wo
  int relu;
  int T;     // > 0: temporal shift over T segments fused into the A loader (1x1, stride 1)
  int fold;  // C / shift_div
  int ntm, ntn;
  int tile;  // 0 = heuristic, else a ConvTile chosen by the engine's autotuner
  int prec;  // ConvPrec: storage format of x, w, res, y and the MFMA used
  // Second A source, concatenated along K behind the first (1x1 convs only): fuses
  //   y = act( conv1x1(x, W) + conv1x1_strided(x2, W2) + bias )
  // i.e. Bottleneck.conv3 + the downsample branch of a stage's first block in one GEMM, so the
  // identity tensor is never written or read.  x2 == nullptr: single source.
  const float *x2;
  int C2, Hi2, Wi2, stride2;
  int K1;    // channels of the first source (its K extent); Kp = K1 + C2
  // Segmented K accumulation (fp32, 64x64 / 32x32 tiles): kseg_len > 0 sums K in consecutive segments of kseg_len
  // K-steps, each from a zero accumulator, and adds the segment sums in order:  out = ((0 + s0) + s1) + ...
  // This fixes the summation order independently of how the work is launched, so the SAME layer can run as one
  // workgroup per tile (ksplit = 0) or as one workgroup per (tile, segment) writing raw partial tiles to
  // y = partial[segment][M][Cout] (ksplit = 1; splitk_reduce then applies bias / residual / ReLU) with
  // bit-identical results: split-K for small batches without giving up batch invariance.
  // ksplit = 2 ("tail split"): output tiles [0, tail_from) run whole-K as with ksplit = 0 and write y; the tiles from
  // tail_from on (a multiple of ntn: whole rows of tiles, i.e. the rows from (tail_from / ntn) * BM to M) run as
  // (tile, segment) workgroups writing ypart = partial[segment][tail rows][Cout], reduced like ksplit = 1's.  For a batch
  // whose tile count leaves the last round of resident workgroups mostly empty: the remainder is spread over the chip in
  // pieces of one K segment.  Same bits as ksplit = 0 / 1.
  int kseg_len;
  int ksplit;
  int tail_from;
  float *ypart;
  // Walk the output tiles from the last one to the first.  The engine alternates this between consecutive launches:
  // a kernel that starts with the rows its predecessor wrote LAST finds them in the 256-MB Infinity Cache / L2.
  int reverse;
  // Position-major rows (segmented fp32 3x3 on 64x64 tiles, pos_major_valid below): GEMM row m' is output position m' / N of
  // frame m' % N, so with N % 64 == 0 a 64-row tile holds ONE output position of 64 frames.  A tap that is padding for that
  // position is padding for the whole tile and its K-steps are not issued at all: they would add +-0 to accumulators that
  // start at +0 and are therefore never -0 (the folded weights are finite), so every bit stays what it is.  A request only:
  // where pos_major_valid does not hold the launch runs in natural order (n, oy, ox).  y and the tail's reduction keep the
  // natural layout [N, Ho, Wo, Cout]; the tail's segment sums (ypart) are in m' order.
  int pos_major;
  // Live-balanced XCD runs of a position-major launch (pos_balanced_runs below).  pos_balance is the request; conv_route answers
  // it and the launcher fills in the rest: pos_whole > 0 = the workgroups of the launch's whole-tile part (8 x the longest run),
  // pos_run[x] .. pos_run[x + 1] = the whole tiles of XCD x.  All zero: equal-count runs.
  int pos_balance;
  int pos_whole;
  int pos_run[9];
};

enum ConvPrec { kPrecF32 = 0, kPrecBf16x3 = 1, kPrecBf16 = 2 };
// (conv_igemm's PREC template argument only: the block-placement arms, a ConvPrec | kPrecBlockShift -- tsm_igemm.hip)
constexpr int kPrecBlockShift = 4;
// (the same: the position-major arm of the segmented fp32 3x3, kPrecF32 | kPrecPosMajor)
constexpr int kPrecPosMajor = 8;

enum ConvTile {
  kTileAuto = 0, kTile128x128 = 1, kTile128x64 = 2, kTile64x64 = 3, kTile32x32 = 4,
  kTile128x128w8 = 5,  // 128x128 on 8 waves (512 threads): same LDS as kTile128x128, twice the waves per SIMD
  kTile256x256 = 6,    // conv_bf16_256_kernel: bf16 only, 8 waves, one workgroup per CU, operands by LDS-DMA
  kTileWs = 7,       // conv3x3_ws[128]_kernel: bf16 3x3 s1 p1 with C = Cout = 64 / 128, weights resident in registers, input patch by LDS-DMA
  kTile256x256p = 8, // conv_bf16_256p_kernel: kTile256x256's pipeline run persistently over a workgroup's tiles (K >= 128, Cout <= 2048)
  kTile64x128 = 9,   // conv_igemm<64, 128, 2, 2, 1, ..>: fp32 unsegmented 1x1 only, a 32x64 wave tile on two accumulators
  kNumTiles = 10
};

// Bottleneck.conv2 (3x3, stride 1, pad 1) + bn2 + ReLU + conv3 (1x1) + bn3 + residual + ReLU as ONE launch (fp32 or split-bf16),
// for CMID = 64 / 128 (layer1 / layer2 blocks without a downsample branch; Cout3 = 4 * CMID), and for CMID = 128 with
// Cout3 = 2 * CMID (wide_resnet50_2's layer1.1-2; conv23_fused2_kernel).  Bit-identical to launch_conv(conv2)
// followed by launch_conv(conv3 with residual).  prec == kPrecBf16: CMID = 64 only, on the weight-stationary kernel
// (conv3x3_ws_kernel<true>); w3f is then conv3's packed weight matrix [256][64] bf16 itself (no fragment packing).
struct Fused23Params {
  const float *x;      // conv2 input [N, H, W, CMID]
  const float *w2;     // [CMID][9 * CMID]  conv2 weights, K = (ky, kx, c), bn2 scale folded in
  const float *bias2;  // [CMID]
  const float *w3f;    // conv3 weights (bn3 scale folded in) in MFMA-fragment order, tsm_host::pack_w3_fragments[_split]
  const float *bias3;  // [Cout3]  (Cout3 = 4 * CMID, or 2 * CMID: launch_conv23_fused's cout3)
  const float *res;    // [M, Cout3]  the block input (identity branch)
  float *y;            // [M, Cout3]
  int N, H, W;
  int M;               // N * H * W
  int kseg_len;        // conv2's K-segment length (ConvParams::kseg_len of that layer; 0 = unsegmented)
  int reverse;         // walk the tiles from the last one to the first (ConvParams::reverse)
};

// A whole Bottleneck of layer1 in ONE launch (bf16, bneck_ws_kernel): temporal shift -> conv1 (1x1, cin -> 64) -> conv2 (3x3) ->
// conv3 (1x1, 64 -> 256) + identity -> ReLU.  cin = 256 (layer1.1 / layer1.2): the identity is the block input, w3 = conv3's
// packed weights [256][64]; cin = 64 (layer1.0): the identity is the downsample branch, K-concatenated behind conv3 as in the
// engine's fused conv3 + downsample GEMM: w3 = [256][64 mid | 64 input] and bias3 = conv3's + the downsample's.  Neither
// 64-channel tensor exists in memory and the block input is streamed once.  Bit-identical to the separate launches.
struct BneckParams {
  const void *x;       // [N, H, W, cin] bf16: the block input (conv1's input through the shift, and the identity operand)
  const void *w1;      // [64][cin] bf16
  const float *bias1;  // [64]
  const void *w2;      // [64][576] bf16, K = (ky, kx, c)
  const float *bias2;  // [64]
  const void *w3;      // [256][64] bf16, or [256][128] with the downsample weights behind conv3's (cin = 64)
  const float *bias3;  // [256]
  void *y;             // [N, H, W, 256] bf16
  int cin;             // 256 or 64
  int N, H, W;
  int T, fold;         // temporal shift over T segments (0 = none), fold = cin / shift_div
  int reverse;         // walk the frames from the last one to the first
};

// Temporal shift + conv1 (1x1, 256 -> 128) + bn1 + ReLU + conv2 (3x3, stride 2, pad 1, 128 -> 128) + bn2 + ReLU of layer2.0 as ONE
// launch (bf16, front_s2_kernel, tsm_front.hip): the 128-channel tensor between the two convolutions never exists in memory.
// Bit-identical to launch_conv(conv1 with shift) followed by launch_conv(conv2).
struct FrontParams {
  const void *x;       // [N, H, W, 256] bf16: the block input
  const void *w1;      // [128][256] bf16, bn1 scale folded in
  const float *bias1;  // [128]
  const void *w2;      // [128][1152] bf16, K = (ky, kx, c), bn2 scale folded in
  const float *bias2;  // [128]
  void *y;             // [N, H / 2, (W - 1) / 2 + 1, 128] bf16: conv2's output
  int N, H, W;
  int T, fold;         // temporal shift over T segments (0 = none), fold = 32
  int reverse;         // walk the frames from the last one to the first
};

// conv3 + bn3 + residual + ReLU of Bottleneck b AND temporal shift + conv1 + bn1 + ReLU of Bottleneck b + 1 as ONE launch
// (bf16, conv31_fused_kernel, tsm_conv31.hip): the block output y is written once (block b + 1's identity) and never read
// back for conv1 -- a tile is all T frames of a clip x 256 / T pixels, so the frames t +- 1 the shifted channels come from
// are rows of the same tile.  Bit-identical to launch_conv(conv3 with residual) followed by launch_conv(conv1 with shift).
struct Conv31Params {
  const void *t2;      // [F * HW, K3] bf16: conv3's input (conv2's output of block b)
  const void *w3;      // [C][K3] bf16, bn3 scale folded in
  const float *bias3;  // [C]
  const void *res;     // [F * HW, C] bf16: block b's input (the identity branch)
  void *y;             // [F * HW, C] bf16: block b's output
  const void *w1;      // [N1][C] bf16: conv1 of block b + 1, bn1 scale folded in
  const float *bias1;  // [N1]
  void *t1;            // [F * HW, N1] bf16: conv1's output of block b + 1
  int n_clips, T, HW;  // F = n_clips * T frames of HW pixels
  int K3, C, N1;
  int fold;            // channels [0, fold) of conv1's input come from frame t + 1, [fold, 2 fold) from t - 1 (0: no shift)
  int reverse;         // walk the tiles from the last one to the first
  int log_px;          // (set by the launcher: log2(256 / T))
};

constexpr int kBK = 32;   // K-step of conv_igemm in channels-taps (bf16: 64)

// ---- tiles ------------------------------------------------------------------------------------------------------------------
inline void conv_tile_dims(int tile, int *bm, int *bn) {
  *bm = (tile == kTile256x256 || tile == kTile256x256p || tile == kTileWs) ? 256 : tile == kTile32x32 ? 32 : ((tile == kTile64x64 || tile == kTile64x128) ? 64 : 128);
  *bn = (tile == kTile256x256 || tile == kTile256x256p) ? 256 : tile == kTile32x32 ? 32 : ((tile == kTile128x128 || tile == kTile128x128w8 || tile == kTile64x128) ? 128 : 64);
}

// "128x128" | "128x64" | "64x64" | "32x32" | "128x128w8" | "256x256" | "256x256p" | "ws" | "64x128" -> ConvTile (kTileAuto for anything else).
inline int conv_tile_from_name(const char *name) {
  if (!name) return kTileAuto;
  static const struct { const char *n; int t; } names[] = {{"128x128", kTile128x128}, {"128x64", kTile128x64},
      {"64x64", kTile64x64}, {"32x32", kTile32x32}, {"128x128w8", kTile128x128w8}, {"256x256", kTile256x256}, {"ws", kTileWs}, {"256x256p", kTile256x256p}, {"64x128", kTile64x128}};
  for (const auto &e : names)
    if (strcmp(name, e.n) == 0) return e.t;
  return kTileAuto;
}

// Number of K segments of a launch with kseg_len > 0 (1 otherwise).
inline int conv_num_segments(const ConvParams &p) {
  if (p.kseg_len <= 0) return 1;
  const int nk = p.Kp / kBK;
  return (int)(((long)nk + p.kseg_len - 1) / p.kseg_len);
}

// Tile rows the heuristics pick (tile == kTileAuto).
inline void conv_tile_shape(const ConvParams &p, int *bm, int *bn) {
  // Cout is a multiple of 64 everywhere in ResNet-50.  Prefer 128x128; fall back to 64x64 when the grid would leave most of the
  // 256 CUs idle (small M at batch 1).
  const int bn128 = p.Cout % 128 == 0 ? 128 : 64;
  const bool few = (((long)p.M + 127) / 128) * (p.Cout / bn128) < 256;
  *bm = few ? 64 : 128;
  *bn = few ? 64 : bn128;
}

// ---- weight-stationary kernels (tsm_ws.hip): LDS budgets and tile geometries ---------------------------------------------------
constexpr int kWsRounds = 11;                    // conv3x3_ws: DMA rounds of 32 patch pixels (4 waves x 8 pixels)
constexpr int kWsPatchMax = kWsRounds * 32;      // 352 patch pixels per buffer (18 x 18 for a 16 x 16 tile, 6 x 58 for 4 x 56)
constexpr int kW8Rounds = 6;                     // conv3x3_ws128, stride 1: DMA rounds of 32 patch pixels per plane
constexpr int kW8PatchMax = kW8Rounds * 32;      // 192 patch pixels (10 x 18 for an 8 x 16 tile, 6 x 30 for 4 x 28)
constexpr int kS2PatchMax = 289;                 // stride 2: 17 x 17 for an 8 x 8 tile (config 5: 32 x 32 outputs), 9 x 29 for 4 x 14 (28 x 28)

// Tile geometry for an H x W frame: TR x TC <= 256 output pixels, (TR + 2) x (TC + 2) <= kWsPatchMax patch pixels,
// fewest tiles per frame (ties: the smaller patch).  Returns false when nothing fits.
inline bool ws_tile_geometry(int H, int W, int *tr_out, int *tc_out, int max_px = 256, int max_patch = kWsPatchMax) {
  long best_tiles = -1;
  int best_tr = 0, best_tc = 0, best_patch = 0;
  for (int tc = 4; tc <= 128; ++tc) {
    int tr = max_px / tc;
    if (tr > H) tr = H;
    if (tr < 1) continue;
    const int patch = (tr + 2) * (tc + 2);
    if (patch > max_patch) continue;
    const long tiles = (((long)H + tr - 1) / tr) * (((long)W + tc - 1) / tc);
    if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && patch < best_patch)) {
      best_tiles = tiles; best_tr = tr; best_tc = tc; best_patch = patch;
    }
  }
  *tr_out = best_tr;
  *tc_out = best_tc;
  return best_tiles > 0;
}

// Stride 2: lanes per tile row of an M-tile pair (64 lanes), and the tile geometry for Ho x Wo outputs: TC <= LPR columns,
// TR <= 64 / LPR rows, (2 TR + 1) x (2 TC + 1) <= kS2PatchMax patch pixels, fewest tiles per frame (ties: the smaller patch).
inline int ws_s2_lanes_per_row(int tc) { return tc <= 8 ? 8 : tc <= 16 ? 16 : tc <= 32 ? 32 : 64; }
inline bool ws_s2_tile_geometry(int Ho, int Wo, int *tr_out, int *tc_out) {
  long best_tiles = -1;
  int best_tr = 0, best_tc = 0, best_patch = 0;
  for (int tc = 1; tc <= 64; ++tc) {
    int tr = 64 / ws_s2_lanes_per_row(tc);
    if (tr > Ho) tr = Ho;
    if (tr < 1) continue;
    const int patch = (2 * tr + 1) * (2 * tc + 1);
    if (patch > kS2PatchMax) continue;
    if (2 * tr * (2 * tc + 1) + ws_s2_lanes_per_row(tc) + tc >= kS2PatchMax) continue;   // idle lanes of a row read behind it: the largest position they form stays <= kS2PatchMax - 1, inside the plane
    const long tiles = (((long)Ho + tr - 1) / tr) * (((long)Wo + tc - 1) / tc);
    if (best_tiles < 0 || tiles < best_tiles || (tiles == best_tiles && patch < best_patch)) {
      best_tiles = tiles; best_tr = tr; best_tc = tc; best_patch = patch;
    }
  }
  *tr_out = best_tr;
  *tc_out = best_tc;
  return best_tiles > 0;
}

// The pixel of lane l31 of M-tile mt (q = 32 mt + l31): its row / column in the tile (row 0x4000: an idle lane) and the patch
// position of its top-left tap.  One definition for the kernel and for the host's bank-conflict model below.
TSM_HOST_DEVICE inline void ws128_lane_pixel(bool s2, int TR, int TC, int PW, int q, int *prow, int *pcol, int *pp0) {
  if (s2) {
    const int lpr = TC <= 8 ? 8 : TC <= 16 ? 16 : TC <= 32 ? 32 : 64;
    const int j = q / lpr, c = q - j * lpr;
    const int r = lpr == 8 ? (j >> 1) + 4 * (j & 1) : j;         // LPR = 8: rows r, r + 4 share a 16-lane group
    const bool ok = r < TR && c < TC;
    *prow = ok ? r : 0x4000;
    *pcol = c;
    *pp0 = (r < TR ? 2 * r * PW : 0) + c;                          // (idle lanes read inside the plane, next to their row's pixels)
  } else {
    const bool ok = q < TR * TC;
    const int r = q / TC, c = q - r * TC;
    *prow = ok ? r : 0x4000;
    *pcol = c;
    *pp0 = ok ? r * PW + c : 0;
  }
}
// Which 16-byte half of its 32-byte plane entry holds k 0-7 of patch position pp (row r = pp / PW, place q = pp % PW in the row):
// half (k >> 3) ^ swap.  A ds_read_b128 is served in four groups of 16 lanes -- lanes {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31} and
// the same + 32 (MI355X_MICROARCH.md, LDS) -- one LDS cycle per group when its 16 lanes hit 16 different 16-byte slots of the
// 256-byte bank row; slot = 2 (pp mod 8) + half ^ swap, so two positions of a group that agree mod 8 must differ in `swap`.
// Round 2-4 swapped on bit 3 of pp, which is conflict-free for 16 CONSECUTIVE positions per group -- not what the hardware's
// groups read: every fragment read of the config-5 tiles was 2-way conflicted (SQ_LDS_BANK_CONFLICT 65 % / 49 % of the LDS
// cycles, profiles/r04_bf16c5_pmc_sq1.txt; the model below says 50 %), at one read per MFMA exactly the matrix pipe's time.
// mode 0: bit 3 of pp; 1: bit 1 of q; 2: bit 0 of r; 3: bit 1 of r.  The host picks the mode with the fewest conflict cycles.
TSM_HOST_DEVICE inline int ws128_swap(int mode, int pp, int PW) {
  const int r = pp / PW, q = pp - r * PW;
  return (mode == 1 ? (q >> 1) : mode == 2 ? r : mode == 3 ? (r >> 1) : (pp >> 3)) & 1;
}
// LDS cycles of the fragment reads of one tile (all M-tiles x 9 taps, one k16 plane) under swap mode `mode`; 4 per read = conflict-free.
inline int ws128_read_cycles(bool s2, int TR, int TC, int mode) {
  static const int kGroup[2][16] = {{0, 1, 2, 3, 12, 13, 14, 15, 20, 21, 22, 23, 24, 25, 26, 27},
                                    {4, 5, 6, 7, 8, 9, 10, 11, 16, 17, 18, 19, 28, 29, 30, 31}};
  const int PW = s2 ? 2 * TC + 1 : TC + 2, kMT = s2 ? 2 : 4;
  int cycles = 0;
  for (int mt = 0; mt < kMT; ++mt)
    for (int tap = 0; tap < 9; ++tap) {
      const int ky = tap / 3, kx = tap - ky * 3;
      for (int half = 0; half < 2; ++half)
        for (int g = 0; g < 2; ++g) {
          int addr[16], worst = 1;
          for (int i = 0; i < 16; ++i) {
            int prow, pcol, pp0;
            ws128_lane_pixel(s2, TR, TC, PW, mt * 32 + kGroup[g][i], &prow, &pcol, &pp0);
            const int pp = pp0 + ky * PW + (s2 ? (kx == 1 ? TC + 1 : kx >> 1) : kx);
            addr[i] = pp * 2 + (half ^ ws128_swap(mode, pp, PW));      // in 16-byte units
          }
          for (int i = 0; i < 16; ++i) {     // distinct addresses on the same slot (equal addresses broadcast)
            int ways = 0;
            for (int k = 0; k < 16; ++k) {
              bool first = (addr[k] & 15) == (addr[i] & 15);
              for (int m = 0; first && m < k; ++m) first = addr[m] != addr[k];
              ways += first ? 1 : 0;
            }
            worst = ways > worst ? ways : worst;
          }
          cycles += worst;
        }
    }
  return cycles;
}
inline int ws128_best_swap(bool s2, int TR, int TC) {
  int best = 0, best_c = ws128_read_cycles(s2, TR, TC, 0);
  for (int mode = 1; mode < 4; ++mode) {
    const int c = ws128_read_cycles(s2, TR, TC, mode);
    if (c < best_c) { best = mode; best_c = c; }
  }
  return best;
}
// The stride-2 tile's swap mode (the same modelling cost as below: the calling thread remembers its last answer).
inline int ws128s2_swap(int tr, int tc) {
  static thread_local int m_tr = 0, m_tc = 0, m_swz = 0;
  if (m_tr != tr || m_tc != tc) { m_swz = ws128_best_swap(true, tr, tc); m_tr = tr; m_tc = tc; }
  return m_swz;
}

// The stride-1 tile of a frame: fewest tiles first (ws_tile_geometry's rule), and among the shapes with that many tiles the one whose
// fragment reads cost the fewest LDS cycles under its best swap -- the shapes differ by a factor of two there: on 32 x 32 frames
// 16 x 8 and 8 x 16 both give 8 tiles, but an M-tile of four 8-pixel rows puts FOUR lanes of a 16-lane read group on one pair of
// 16-byte slots (two entries per slot pair: 2-way conflicts whatever the swap, 50 % of the LDS cycles), while two 16-pixel rows
// with the halves swapped on the row's parity read conflict-free.
inline bool ws128_tile_geometry(int H, int W, int *tr_out, int *tc_out, int *swz_out) {
  // (a pure function of the frame size, but ~10^7 operations of modelling: every launch of an engine asks for the same one or
  //  two sizes, so the calling thread remembers its last four answers)
  struct Memo { int H, W, tr, tc, swz; bool ok; };
  static thread_local Memo memo[4] = {};
  static thread_local int memo_next = 0;
  for (const Memo &m : memo)
    if (m.H == H && m.W == W && m.H > 0) {
      *tr_out = m.tr; *tc_out = m.tc;
      if (swz_out) *swz_out = m.swz;
      return m.ok;
    }
  long best_tiles = -1;
  int best_tr = 0, best_tc = 0, best_cycles = 0, best_swz = 0;
  for (int tc = 4; tc <= 128; ++tc) {
    int tr = 128 / tc;
    if (tr > H) tr = H;
    if (tr < 1 || (tr + 2) * (tc + 2) > kW8PatchMax) continue;
    const long tiles = (((long)H + tr - 1) / tr) * (((long)W + tc - 1) / tc);
    if (best_tiles >= 0 && tiles > best_tiles) continue;
    const int swz = ws128_best_swap(false, tr, tc), cycles = ws128_read_cycles(false, tr, tc, swz);
    if (best_tiles < 0 || tiles < best_tiles || cycles < best_cycles) {
      best_tiles = tiles; best_tr = tr; best_tc = tc; best_cycles = cycles; best_swz = swz;
    }
  }
  *tr_out = best_tr;
  *tc_out = best_tc;
  if (swz_out) *swz_out = best_swz;
  memo[memo_next] = Memo{H, W, best_tr, best_tc, best_swz, best_tiles > 0};
  memo_next = (memo_next + 1) & 3;
  return best_tiles > 0;
}

// Tiles of n frames of h x w output pixels cut into tr x tc tiles.
inline long ws_frame_tiles(int n, int h, int w, int tr, int tc) { return (long)n * (((long)h + tr - 1) / tr) * (((long)w + tc - 1) / tc); }
// Grid of a persistent kernel: one workgroup per CU, or per tile where there are fewer.
inline unsigned persistent_grid(long tiles, int n_cu) { return (unsigned)(tiles < n_cu ? tiles : n_cu); }

// ---- does a kernel family apply?  (shapes, and the null-ness of res / x2) ----------------------------------------------------
// conv_bf16_256_kernel (kTile256x256)
inline bool conv_bf16_256_valid(const ConvParams &p, int ks) {
  if (p.prec != kPrecBf16 || (ks != 1 && ks != 3) || p.Cout % 256 != 0 || p.C % 64 != 0 || p.Kp % 64 != 0 || p.kseg_len != 0)
    return false;
  if (ks == 3) return !p.res && !p.x2 && p.T == 0;
  if (p.T > 0) return !p.res && !p.x2;                    // shifted conv1
  if (p.x2) return !p.res && p.K1 % 64 == 0 && p.C2 % 64 == 0;
  return true;
}
// conv_bf16_256p_kernel (kTile256x256p): at least two K-tiles per tile, the bias of all channels in LDS
inline bool conv_bf16_256p_valid(const ConvParams &p, int ks) {
  if (ks == 1 && p.T > 0 && (p.res || p.x2)) {   // block placement: the shifted identity / second source (8-channel chunks)
    ConvParams q = p;
    q.T = 0;
    return conv_bf16_256p_valid(q, ks) && p.N % p.T == 0 && p.fold % 8 == 0 && 2 * (int64_t)p.fold <= (p.res ? p.Cout : p.C2);
  }
  return conv_bf16_256_valid(p, ks) && p.Kp >= 128 && p.Cout <= 2048;
}

// The weight-stationary 3x3 kernels; each rule also gives the tile geometry it found (tr, tc; swz: the swap mode of ws128).
// conv3x3_ws_kernel<false>: 3x3 s1 p1, 64 -> 64 channels (Bottleneck.conv2 of layer1)
inline bool conv3x3_ws_valid(const ConvParams &p, int *tr, int *tc) {
  return p.prec == kPrecBf16 && p.C == 64 && p.Cout == 64 && p.Kp == 576 && p.stride == 1 && p.pad == 1 && p.Hi == p.Ho &&
         p.Wi == p.Wo && !p.res && !p.x2 && p.T == 0 && p.kseg_len == 0 && (double)p.M * 128.0 < 2.0e9 &&
         ws_tile_geometry(p.Hi, p.Wi, tr, tc);
}
// conv3x3_ws128_kernel: 3x3 p1, 128 -> 128 channels, stride 1 or (layer2.0's conv2) stride 2
inline bool conv3x3_ws128_common(const ConvParams &p) {
  return p.prec == kPrecBf16 && p.C == 128 && p.Cout == 128 && p.Kp == 1152 && p.pad == 1 && !p.res && !p.x2 && p.T == 0 &&
         p.kseg_len == 0 && (double)p.M * 256.0 < 2.0e9 && (double)p.Hi * p.Wi * 256.0 < 2.0e9;
}
inline bool conv3x3_ws128s2_valid(const ConvParams &p, int *tr, int *tc) {
  return conv3x3_ws128_common(p) && p.stride == 2 && p.Ho == (p.Hi - 1) / 2 + 1 && p.Wo == (p.Wi - 1) / 2 + 1 && p.Wi <= 2048 &&
         ws_s2_tile_geometry(p.Ho, p.Wo, tr, tc);
}
inline bool conv3x3_ws128_valid(const ConvParams &p, int *tr, int *tc, int *swz) {
  return conv3x3_ws128_common(p) && p.stride == 1 && p.Hi == p.Ho && p.Wi == p.Wo && ws128_tile_geometry(p.Hi, p.Wi, tr, tc, swz);
}

// conv1x1_ws_kernel: 1x1, 64 / 256 -> 64 channels, optional fused temporal shift (layer1's conv1)
inline bool conv1x1_ws_valid(const ConvParams &p) {
  return p.prec == kPrecBf16 && (p.C == 64 || p.C == 256) && p.Cout == 64 && p.Kp == p.C && p.stride == 1 && p.pad == 0 &&
         p.Hi == p.Ho && p.Wi == p.Wo && !p.res && !p.x2 && p.kseg_len == 0 && (double)p.M * 128.0 < 2.0e9 &&
         (p.T == 0 || (p.N % p.T == 0 && p.fold % 8 == 0 && 2 * (int64_t)p.fold <= p.C)) &&
         (double)(128 + 2.0 * p.Hi * p.Wi) * p.C * 2.0 < 2.0e9;
}
// conv1x1_wsn_kernel: 1x1 to 128 / 256 channels (conv1 of layer2 / layer3.0, conv3 + downsample of layer1.0 / layer2.0).  The
// two-halves form of layer2.0 runs workgroup PAIRS in multiples of 8: it needs 16 CUs.
inline bool conv1x1_wsn_valid(const ConvParams &p, int n_cu) {
  if (p.prec != kPrecBf16 || p.stride != 1 || p.pad != 0 || p.Hi != p.Ho || p.Wi != p.Wo || p.res || p.kseg_len != 0) return false;
  if ((double)(128 + 2.0 * p.Hi * p.Wi) * p.C * 2.0 >= 2.0e9) return false;
  if (p.x2) {   // conv3 + downsample of layer1.0: 64 + 64 -> 256; of layer2.0: 128 + 256 -> 512 (two halves of 256)
    const bool l1 = p.C == 64 && p.C2 == 64 && p.K1 == 64 && p.Kp == 128 && p.Cout == 256;
    const bool l2 = p.C == 128 && p.C2 == 256 && p.K1 == 128 && p.Kp == 384 && p.Cout == 512 && n_cu >= 16;
    return p.T == 0 && (l1 || l2) && (double)(128.0 / ((double)p.Hi * p.Wi) + 2.0) * p.Hi2 * p.Wi2 * p.C2 * 2.0 < 2.0e9;
  }
  if (p.Kp != p.C) return false;
  if (p.T > 0 && (p.N % p.T != 0 || p.fold % 8 != 0 || 2 * (int64_t)p.fold > p.C)) return false;
  return (p.C == 256 && p.Cout == 128) || (p.C == 512 && p.Cout == 128) || (p.C == 512 && p.Cout == 256);
}

// May the tuner offer `tile` for this problem, and does checked_code trust a cached code with it?  A necessary condition of
// conv_route accepting the launch with p.tile = tile, not always a sufficient one ("Known gap").
inline bool conv_tile_valid(const ConvParams &p, int tile, int n_cu) {
  // Block placement's arms (a shifted identity or second source, a shifted 1x1 at stride 2) exist on conv_igemm's tiles, and for
  // a 1x1's shifted identity / second source on the persistent 256x256 tile (conv_bf16_256p_kernel<1, true, RES, DUAL>).
  if (p.T > 0 && (p.res || p.x2 || (p.pad == 0 && p.stride != 1)) &&
      (tile == kTile256x256 || tile == kTileWs || (tile == kTile256x256p && (p.pad != 0 || !(p.res || p.x2)))))
    return false;
  switch (tile) {
    case kTile128x128: return p.Cout % 128 == 0;
    case kTile128x64:
    case kTile64x64: return p.Cout % 64 == 0;
    case kTile32x32: return p.Cout % 32 == 0 && p.prec == kPrecF32;  // single-wave tiles: fp32 only
    case kTile128x128w8: return p.Cout % 128 == 0;
    // The 256 tiles, NOT as conv_bf16_256[p]_valid say it: this question has no ks (the pad stands in for it: a 3x3 (pad 1) only
    // unshifted and without a residual; the stem has C == 4 and never qualifies), and it ignores Kp % 64, kseg_len and, for 256p's
    // block-placement arms, N % T, fold % 8 and 2 fold <= the shifted channels, which conv_route checks.
    case kTile256x256:
    case kTile256x256p:   // (256p: at least two K-tiles, the bias of all channels in LDS)
      return p.prec == kPrecBf16 && p.Cout % 256 == 0 && p.C % 64 == 0 && !(p.res && p.x2) && (p.pad != 1 || (!p.res && p.T == 0)) &&
             (!p.x2 || (p.K1 % 64 == 0 && p.C2 % 64 == 0)) && (tile == kTile256x256 || (p.Cout <= 2048 && p.Kp >= 128));
    // 64x128: fp32, a 1x1 (no padding), unsegmented, no block placement (a shifted identity / second source / strided 1x1)
    case kTile64x128:
      return p.prec == kPrecF32 && p.pad == 0 && p.kseg_len == 0 && p.Cout % 128 == 0 &&
             !(p.T > 0 && (p.res || p.x2 || p.stride != 1));
    case kTileWs: {   // (pad singles out 3x3 / 1x1)
      int tr, tc;
      return conv3x3_ws_valid(p, &tr, &tc) || conv3x3_ws128s2_valid(p, &tr, &tc) || conv3x3_ws128_valid(p, &tr, &tc, nullptr) ||
             conv1x1_ws_valid(p) || conv1x1_wsn_valid(p, n_cu);
    }
    default: return false;
  }
}

// ---- the route of a launch_conv call ---------------------------------------------------------------------------------------------
// The kernel family of a route: refused (nothing is launched) | conv_igemm | conv_igemm<..., SEG = true> (segmented K: fp32, 64x64 /
// 32x32, no residual) | conv_bf16_256_kernel | conv_bf16_256p_kernel | conv3x3_ws_kernel<false> | conv3x3_ws128_kernel<false> |
// conv3x3_ws128_kernel<true> (stride 2) | conv1x1_ws_kernel | conv1x1_wsn_kernel
enum ConvFamily { kFamInvalid = 0, kFamIgemm, kFamIgemmSeg, kFamBf16_256, kFamBf16_256p, kFamWs3x3, kFamWs128, kFamWs128s2, kFamWs1x1, kFamWsn };

struct ConvRoute {
  int family = kFamInvalid, ks = 0;
  int bm = 0, bn = 0, wgm = 0, wgn = 0;   // tile and wave grid (igemm families, 256 / 256p)
  // The template arm.  igemm: the launcher's <KS, SHIFT, RES> -- shift = the A operand through the temporal shift, res = a
  // residual -- dual = a second source, block_shift = block placement: the identity (residual or second source) through the
  // shift, conv_igemm<.., false, false, PREC | kPrecBlockShift(, true)>, which adds the residual itself.  256 / 256p: their
  // <KS, SHIFT, RES, DUAL>.
  bool shift = false, res = false, dual = false, block_shift = false;
  bool pos_major = false;   // kFamIgemmSeg only: the position-major arm, conv_igemm<64, 64, 2, 2, 3, .., kPrecF32 | kPrecPosMajor, false, true>
  int ntm = 0, ntn = 0;   // what the launcher puts into ConvParams (igemm families, 256 / 256p)
  long tiles = 0;         // output tiles (the segmented forms launch up to conv_num_segments workgroups for each)
  unsigned grid = 0;      // workgroups
  int tr = 0, tc = 0, swz = 0;   // weight-stationary 3x3 geometry
  // pos_major with ConvParams::pos_balance: the whole-tile workgroups (8 x the longest run; 0 = equal-count runs) and the runs
  int pos_whole = 0, pos_run[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
};

// launch_conv's argument rules: true when the launch is refused whatever the tile.
inline bool conv_args_refused(const ConvParams &p, int ks) {
  const int kc = p.prec == kPrecBf16 ? 64 : kBK;  // channels per K-step
  if (p.Cout % 64 != 0 || p.Kp % kc != 0 || p.M <= 0) return true;
  if (p.logC4 < 0 || p.logC4 > 28 || (1 << p.logC4) * 4 != p.C) return true;
  if (ks != 7 && p.C % kc != 0) return true;
  // temporal shift of the A operand: 1x1 (Bottleneck.conv1; stride 2: BasicBlock downsample under block placement), 3x3 at
  // stride 1 or 2 (BasicBlock.conv1; unsegmented only).  With a residual or a second source (block placement) T shifts the
  // identity / x2 instead, fold = its channels / shift_div.
  if (p.T > 0 && ((ks != 1 && ks != 3) || (ks == 3 && p.kseg_len > 0) || p.N % p.T != 0 || p.fold % 4 != 0 ||
                  (p.res && 2 * (int64_t)p.fold > p.Cout) || (p.x2 && 2 * (int64_t)p.fold > p.C2)))
    return true;
  if (p.x2 && (ks != 1 || p.res || p.K1 % kc != 0 || p.C2 % kc != 0 || (int64_t)p.K1 + p.C2 != p.Kp || p.K1 != p.C))
    return true;
  // the second source's window: the frames of a tile (one more before it when shifted), through 32-bit offsets
  if (p.x2 && (128.0 / ((double)p.Ho * p.Wo) + 4.0) * (double)p.Hi2 * p.Wi2 * p.C2 * 4.0 > 2.0e9) return true;
  // a shifted identity reads rows up to one frame either side of the tile through 32-bit offsets
  if (p.T > 0 && p.res && (128.0 + 2.0 * p.Ho * p.Wo) * p.Cout * 4.0 > 2.0e9) return true;
  if (p.prec != kPrecF32 && p.prec != kPrecBf16x3 && p.prec != kPrecBf16) return true;
  if (p.kseg_len < 0 || (p.kseg_len > 0 && (p.prec != kPrecF32 || p.res || ks == 7))) return true;
  if ((p.ksplit && p.kseg_len <= 0) || p.ksplit < 0 || p.ksplit > 2) return true;
  if (p.prec != kPrecF32 && p.T > 0 && p.fold % 8 != 0) return true;
  // stem: 4 channels per pixel (3 + a zero); the bf16 formats read pixel pairs, which needs stride 2 / pad 3
  if (ks == 7 && (p.C != 4 || (p.prec != kPrecF32 && (p.stride != 2 || p.pad != 3)))) return true;
  // 32-bit byte offsets inside a workgroup's rebased window: a tile touches at most BM/(Ho*Wo) + 4 input frames.
  if ((128.0 / ((double)p.Ho * p.Wo) + 4.0) * (double)p.Hi * p.Wi * p.C * 4.0 > 2.0e9) return true;
  return (ks != 1 && ks != 3 && ks != 7) || (ks == 7 && p.res);
}

// ---- position-major rows (ConvParams::pos_major): what the kernel and the split reduction compute, callable on the CPU --------
// GEMM row m of a position-major launch over n_frames frames: its frame and its output position.  m -> frame * HoWo + pos (the
// row of y it is stored to) is a bijection of [0, n_frames * HoWo).
TSM_HOST_DEVICE inline void pos_major_row(int m, int n_frames, int *frame, int *pos) {
  *pos = m / n_frames;
  *frame = m - *pos * n_frames;
}
// Bit ky * 3 + kx is set when tap (ky, kx) of output position `pos` reads inside the Hi x Wi frame; a clear bit is a tap of the
// zero padding, for every frame alike.
TSM_HOST_DEVICE inline unsigned pos_major_tap_mask(int pos, int Wo, int Hi, int Wi, int stride, int pad) {
  const int oy = pos / Wo, ox = pos - oy * Wo;
  const int iy0 = oy * stride - pad, ix0 = ox * stride - pad;
  unsigned mask = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx)
      if ((unsigned)(iy0 + ky) < (unsigned)Hi && (unsigned)(ix0 + kx) < (unsigned)Wi) mask |= 1u << (ky * 3 + kx);
  return mask;
}
// The first K-step in [kt, nk) whose tap is set in `mask`, or nk when there is none.  K is ordered (ky, kx, c): tap t owns the
// K-steps [t, t + 1) * steps_per_tap, steps_per_tap = C / 32, a power of two (ConvParams::logC4).
TSM_HOST_DEVICE inline int next_live_kstep(int kt, unsigned mask, int steps_per_tap, int nk) {
  if (kt < 0 || kt >= nk) return nk;
  const int log_spt = __builtin_ctz((unsigned)steps_per_tap);
  const int tap = kt >> log_spt;
  const unsigned rest = tap < 9 ? (mask & 0x1ffu) >> tap : 0u;
  if (rest & 1u) return kt;
  if (rest == 0u) return nk;
  const int next = (tap + __builtin_ctz(rest)) << log_spt;
  return next < nk ? next : nk;
}
// May this launch run position-major?  Everything the arm assumes: one output position per 64-row tile and no row past M
// (N % 64 == 0), whole taps per K-step, y and all N input frames inside one buffer descriptor (2 GB).
inline bool pos_major_valid(const ConvParams &p, int ks) {
  return p.prec == kPrecF32 && ks == 3 && p.pad == 1 && (p.stride == 1 || p.stride == 2) && p.kseg_len > 0 && p.T == 0 &&
         !p.res && !p.x2 && (p.tile == kTile64x64 || p.tile == kTileAuto) && (p.ksplit == 0 || p.ksplit == 2) &&
         p.N > 0 && p.N % 64 == 0 && p.Ho > 0 && p.Wo > 0 && (int64_t)p.N * p.Ho * p.Wo == p.M &&
         p.C >= kBK && (p.C & (p.C - 1)) == 0 && p.Kp == (int64_t)9 * p.C &&
         (double)p.N * p.Hi * p.Wi * p.C * 4.0 < 2.0e9 && (double)p.M * p.Cout * 4.0 < 2.0e9;
}

// Live-balanced XCD runs.  conv_igemm gives XCD x (workgroups x, x + 8, ..) a contiguous run of tiles; with equal tile counts the
// runs of a position-major launch differ in work, because a tile costs its position's live taps (4, 6 or 9 of 9) and the runs
// holding the first and last rows of positions are light -- the launch then ends with its heaviest XCD.  This cuts the whole
// tiles [0, nwg) (nwg % ntn == 0; tile order unchanged: n fastest, frame group, position) into 8 contiguous runs at multiples
// of ntn (the n-tiles of one A panel stay together), boundary k at the tile group where the cumulative live taps come closest
// to k / 8 of the total: every boundary is within half a tile group's cost of its target, so every run's live work lies within
// one tile group (ntn tiles x 9 taps) of total / 8.  run[0] = 0 .. run[8] = nwg; returns 8 x the longest run: the workgroups of
// the whole-tile part (the hardware deals workgroups evenly, so each XCD gets the longest run's count and a workgroup past its
// own run's end returns at once).  Fewer tile groups than XCDs: some runs are empty.
constexpr int kXcds = 8;
inline int pos_balanced_runs(const ConvParams &p, int ntn, long nwg, int run[kXcds + 1]) {
  const int groups = (int)(nwg / ntn), per_pos = p.N / 64;   // (pos_major_valid: N % 64 == 0, a tile group is one position's 64 frames)
  int cached_pos = -1, cached_cost = 0;
  auto cost = [&](int g) {
    const int pos = g / per_pos;
    if (pos != cached_pos) {
      cached_pos = pos;
      cached_cost = __builtin_popcount(pos_major_tap_mask(pos, p.Wo, p.Hi, p.Wi, p.stride, p.pad));
    }
    return cached_cost;
  };
  long total = 0;
  for (int g = 0; g < groups; ++g) total += cost(g);
  long cum = 0;   // the live taps of the groups [0, g)
  int g = 0, longest = 0;
  run[0] = 0;
  for (int k = 1; k <= kXcds; ++k) {
    int b = groups;
    if (k < kXcds) {
      while (g < groups && cum * kXcds < k * total) cum += cost(g++);
      b = g;   // the first boundary at or past the target; the one before it when that is closer
      if (g > 0 && k * total - (cum - cost(g - 1)) * kXcds < cum * kXcds - k * total) b = g - 1;
    }
    run[k] = b * ntn;
    if (run[k] - run[k - 1] > longest) longest = run[k] - run[k - 1];
  }
  return kXcds * longest;
}

// ks in {1, 3, 7}; n_cu sizes the persistent grids (read by the 256p and weight-stationary families only).  A grid past 2^31 - 1
// workgroups is refused (the products are formed in 64 bits; in 32 they were a signed overflow).
inline ConvRoute conv_route(const ConvParams &p, int ks, int n_cu) {
  ConvRoute r, refused;
  if (conv_args_refused(p, ks) || (p.tile != kTileAuto && !conv_tile_valid(p, p.tile, n_cu))) return refused;
  r.ks = ks; r.res = p.res != nullptr; r.dual = p.x2 != nullptr;
  r.shift = !r.res && p.T > 0 && !(ks == 1 && r.dual);   // (with a residual or a second source, T > 0 shifts THAT: block placement)
  if (p.tile == kTileAuto) conv_tile_shape(p, &r.bm, &r.bn);
  else conv_tile_dims(p.tile, &r.bm, &r.bn);
  if (p.tile == kTile256x256 || p.tile == kTile256x256p) {
    const bool persistent = p.tile == kTile256x256p;
    if (!(persistent ? conv_bf16_256p_valid(p, ks) : conv_bf16_256_valid(p, ks))) return refused;
    r.family = persistent ? kFamBf16_256p : kFamBf16_256;
    r.wgm = 2; r.wgn = 4;
    r.shift = ks == 1 && p.T > 0;   // (256p: of the A operand, or with res / dual of the identity / second source)
    r.ntm = (int)(((long)p.M + 255) / 256); r.ntn = p.Cout / 256;
    r.tiles = (long)r.ntm * r.ntn;
    const int slots = n_cu & ~7;    // 256p: a multiple of 8: a workgroup's tiles then all sit in its own XCD's chunk
    r.grid = (unsigned)(!persistent || r.tiles < slots || slots < 8 ? r.tiles : slots);
    return r.tiles > 0x7fffffffL ? refused : r;
  }
  if (p.tile == kTileWs) {   // persistent, a workgroup per CU: 3x3 by frame tiles, 1x1 by tiles of 128 (K > 256: 64) pixels
    if (ks == 3) {
      r.family = conv3x3_ws128s2_valid(p, &r.tr, &r.tc) ? kFamWs128s2 : conv3x3_ws128_valid(p, &r.tr, &r.tc, &r.swz) ? kFamWs128 :
                 conv3x3_ws_valid(p, &r.tr, &r.tc) ? kFamWs3x3 : kFamInvalid;
      if (r.family == kFamInvalid) return refused;
      if (r.family == kFamWs128s2) r.swz = ws128s2_swap(r.tr, r.tc);
      r.tiles = ws_frame_tiles(p.N, p.Ho, p.Wo, r.tr, r.tc);
    } else {
      r.family = ks != 1 || r.res ? kFamInvalid : conv1x1_ws_valid(p) ? kFamWs1x1 : conv1x1_wsn_valid(p, n_cu) ? kFamWsn : kFamInvalid;
      if (r.family == kFamInvalid) return refused;
      const int px = r.family == kFamWs1x1 || p.Kp <= 256 ? 128 : 64;
      r.tiles = ((long)p.M + px - 1) / px;
    }
    r.grid = persistent_grid(r.tiles, n_cu);
    if (r.family == kFamWsn && p.x2 && p.Kp == 384) {   // two halves of the output channels per pixel tile
      const int pairs = n_cu >> 4 << 3;                                          // workgroup pairs: a multiple of 8 (b and b + 8 share an XCD)
      r.grid = 2u * (unsigned)(r.tiles < pairs ? (r.tiles + 7) / 8 * 8 : pairs);   // (a pair without a tile leaves at once)
    }
    return r;
  }
  // conv_igemm
  if (p.tile == kTile64x128 && ks != 1) return refused;   // (conv_tile_valid has no ks: a 3x3 or the stem without padding)
  if (p.kseg_len > 0 && r.bm != 32) r.bm = r.bn = 64;   // segmented accumulation exists on 64x64 / 32x32 tiles only
  if (r.bm == 32 && p.prec != kPrecF32) return refused;
  r.wgm = r.bm == 32 ? 1 : r.bm == 128 && r.bn == 128 && p.tile == kTile128x128w8 ? 4 : 2;
  r.wgn = r.bm == 32 ? 1 : 2;
  r.ntm = (int)(((long)p.M + r.bm - 1) / r.bm); r.ntn = p.Cout / r.bn;
  r.tiles = (long)r.ntm * r.ntn;
  long grid = r.tiles;
  if (p.kseg_len > 0) {   // one workgroup per tile, or per (tile, segment) when ksplit is set (2: from tile tail_from on)
    if (r.res || ks == 7 || (r.shift && ks == 3)) return refused;
    if (p.ksplit == 2 && (p.tail_from <= 0 || p.tail_from >= r.tiles || p.tail_from % r.ntn != 0)) return refused;
    r.family = kFamIgemmSeg;
    r.pos_major = p.pos_major != 0 && r.bm == 64 && pos_major_valid(p, ks);   // (anything else: natural order, the same bits)
    grid = p.ksplit == 2 ? p.tail_from + (r.tiles - p.tail_from) * conv_num_segments(p) : r.tiles * (p.ksplit ? conv_num_segments(p) : 1);
    if (r.pos_major && p.pos_balance) {   // live-balanced runs: the whole part grows to 8 x the longest run, the pieces follow it
      const long whole = p.ksplit == 2 ? p.tail_from : r.tiles;
      r.pos_whole = pos_balanced_runs(p, r.ntn, whole, r.pos_run);
      grid += r.pos_whole - whole;
    }
  } else {
    r.family = kFamIgemm;
  }
  r.block_shift = p.T > 0 && (r.dual || r.res);   // block placement: the identity / downsample operand through the shift
  r.grid = (unsigned)grid;
  return grid > 0x7fffffffL ? refused : r;
}

// ---- the fused forms (their launchers: tsm_ws.hip, tsm_bneck.hip, tsm_front.hip, tsm_conv31.hip) --------------------------------
// conv2 + conv3 + residual on conv3x3_ws_kernel<true> (bf16, CMID = 64): n frames of h x w pixels
inline bool conv23_ws_valid(int n, int h, int w, int *tr_out = nullptr, int *tc_out = nullptr) {
  int tr, tc;
  return n > 0 && h > 0 && w > 0 && (double)h * w * 512.0 < 2.0e9 && (double)n * h * w < 2.0e9 &&
         ws_tile_geometry(h, w, tr_out ? tr_out : &tr, tc_out ? tc_out : &tc);
}
inline bool bneck_ws_valid(int cin, int n, int h, int w, int T, int fold) {
  return (cin == 256 || cin == 64) && n > 0 && h > 0 && w >= 1 && w <= 64 && (double)h * w * 512.0 * 3.0 < 2.0e9 &&
         (T == 0 || (T > 0 && n % T == 0 && fold == cin / 8));
}
inline bool front_s2_valid(int n, int h, int w, int T, int fold) {
  return n > 0 && h >= 2 && (h & 1) == 0 && w >= 2 && w <= 64 && (double)h * w * 512.0 * 3.0 < 2.0e9 &&
         (T == 0 || (T > 0 && n % T == 0 && fold == 32));
}
// conv31's instantiations: (K3, C, N1) = (128, 512, 128) layer2.k -> layer2.k+1 on conv31_fused_kernel (tiles of 256 rows);
// (128, 512, 256) layer2.3 -> layer3.0 and (256, 1024, 256) layer3.k -> layer3.k+1 on conv31_pc_kernel (tiles of 128 rows).
inline int conv31_rows(const Conv31Params &p) {
  if (p.K3 == 128 && p.C == 512 && p.N1 == 128) return 256;
  if ((p.K3 == 128 && p.C == 512 && p.N1 == 256) || (p.K3 == 256 && p.C == 1024 && p.N1 == 256)) return 128;
  return 0;
}
inline bool conv31_valid(const Conv31Params &p) {
  const int m = conv31_rows(p);
  if (m == 0) return false;
  if (p.n_clips <= 0 || p.HW <= 0 || p.T <= 0 || m % p.T != 0 || m / p.T < 8) return false;
  if (p.fold != 0 && (p.fold % 64 != 0 || 2 * (int64_t)p.fold > p.C)) return false;  // a 64-channel chunk is shifted as a whole
  return (double)p.T * p.HW * p.C * 2.0 < 2.0e9;                             // 32-bit offsets inside a clip's block
}

}  // namespace tsm
