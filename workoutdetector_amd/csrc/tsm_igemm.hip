// Hand-written CDNA4 (gfx950) kernels for the TSM-ResNet50 clip forward.
//
//   conv_igemm       implicit-GEMM convolution (1x1 / 3x3 / 7x7, stride 1|2), NHWC activations, LDS-staged A
//                    (im2col rows built on the fly, temporal shift fused into the 1x1 and 3x3 loaders) and B (packed
//                    weights), epilogue = folded-BN bias + residual + ReLU.  Template axes: tile shape and wave
//                    layout (128x128 on 4 or 8 waves, 128x64, 64x64, 64x128 for fp32 1x1 convs, 32x32 on one wave), KS, SHIFT (fused
//                    temporal shift), RES (residual prefetched under the K loop), PREC (exact-fp32 MFMA /
//                    split-bf16 x3 / bf16), DUAL (second A source concatenated along K = conv3 + downsample in
//                    one GEMM), SEG (fp32 long-K layers: K summed in fixed segments, which makes whole-K and split-K
//                    launches of a layer bit-identical; splitk_reduce adds the segment sums in order).
//                    Every variant accumulates each output in the same k order: results are bit-identical
//                    across tile shapes, pipelines and launch forms of one precision.
//   pack_input       [N,3,H,W] or [N,H,W,3] fp32 -> the stem's input format (fp32: one 4-channel group per pixel;
//                    bf16 formats: one 8-element group per pixel pair)
//   preprocess       fused test transform: uint8/fp32 frames -> resize 256 / crop 224 / normalise -> packed input
//   maxpool3x3s2     NHWC, any storage format
//   temporal_shift   stand-alone NHWC fp32 shift (tests; the forward uses the fused loader)
//   head             per-frame global avg-pool, then mean over segments + FC
//
// Reference semantics: workoutdetector/models/tsm.py:35-50 (shift), :409-419 (forward/head);
// torchvision-0.13 ResNet-50 v1.5 Bottleneck for the conv stack.
#include "tsm_device.h"

namespace tsm {

// ---------------------------------------------------------------------------------------------
// Implicit-GEMM convolution.  GEMM view: Y[M, Cout] = A[M, K] * W^T[K, Cout],
//   M = N*Ho*Wo output pixels, K = KS*KS*C ordered (ky, kx, c) so that NHWC input rows are
//   contiguous along K within one tap.  One workgroup = WGM x WGN waves (4, 8 or 1), block tile
//   BM x BN, K-step = one 128-byte row per operand (32 fp32 or split channels, 64 bf16 channels).
//   Each wave owns (BM/WGM) x (BN/WGN) as TM x TN MFMA tiles of 32x32.
//
// MFMA operand order: v_mfma_f32_32x32x2_f32 takes A[i = lane&31][k = lane>>5] and
// B[k = lane>>5][j = lane&31].  The reduction order inside K is free as long as A and B agree, so
// each lane fetches FOUR consecutive k (one ds_read_b128) at k = 8*kk + 4*(lane>>5) + s and step s
// of the group multiplies element s: per 8 k, one b128 per operand tile feeds 4 MFMAs.
//
// Loader: branch-free.  Both operands come through raw buffer loads whose descriptor is rebased per
// workgroup (so 32-bit byte offsets always suffice) and whose hardware range check returns zeros
// for an offset of kInvalid: im2col padding, rows past M and the zero frames of the temporal shift
// cost a v_cndmask on the offset instead of a branch.  Everything that depends only on the row
// (pixel decode, padding mask, shift validity) is computed once per thread before the K loop.
//
// Epilogue: accumulators go through LDS once so that global traffic is 16 B per lane along Cout
// (residual read, bias, ReLU, store), i.e. whole 128-B lines instead of 4-B scalars.
// ---------------------------------------------------------------------------------------------
// PREC selects the arithmetic:
//   kPrecF32     activations/weights fp32, v_mfma_f32_32x32x2_f32 (bit-for-bit an fp32 fma chain)
//   kPrecBf16x3  "split-bf16": every value is stored as hi = bf16(x), lo = bf16(x - hi), 8 channels per
//                32-byte group [hi x8 | lo x8] (same 4 bytes per element, same byte offsets as fp32, so the
//                loader is shared).  a*b ~= ah*bh + ah*bl + al*bh on v_mfma_f32_32x32x16_bf16 with fp32
//                accumulation: relative error ~2^-17 per product, three MFMAs at 16x the fp32-MFMA rate.
//
// BSHIFT (block placement, shift_place 'block': the block input is shifted as a whole, so its identity path reads the shifted
// tensor too): the temporal shift moves from the A loader to the identity -- the residual (RES: row r of the identity reads
// row r +- Ho*Wo per channel chunk, p.fold = Cout / shift_div) or the second source of a DUAL GEMM (the downsample operand
// gets the A loader's per-chunk frame choice, p.fold = C2 / shift_div; the first source stays unshifted).  p.T > 0 selects
// it at launch.  Instantiated as PREC | kPrecBlockShift with SHIFT = RES = false (DUAL = false: the shifted residual), so that
// every other instantiation keeps its name and its code.
//
// POSM (position-major rows, ConvParams::pos_major): the segmented fp32 3x3 on 64x64 tiles with GEMM row m' = output position
// m' / N of frame m' % N.  N % 64 == 0 (pos_major_valid), so a tile is ONE output position of 64 frames: the padding mask is a
// wave-uniform scalar, the per-row mask registers and the per-load select go, and the K loop walks the live taps' K-steps only
// (next_live_kstep) -- a padding tap's MFMAs would add +-0 to accumulators that are never -0.  Instantiated as PREC |
// kPrecPosMajor on <64, 64, 2, 2, 3, false, false, .., false, true> alone, like BSHIFT, for the same reason.
template <int BM, int BN, int WGM, int WGN, int KS, bool SHIFT, bool RES, int PREC, bool DUAL = false, bool SEG = false>
// (second launch-bounds argument = minimum waves per SIMD: the SEG 64x64 kernel needs 16 registers more than the
// plain one and would drop from 5 to 4 workgroups per CU; asking for 5 costs 1-2 spills outside the K loop)
// (the 64x128 tile asks for 4: 128 registers, 4 workgroups of 27 KB per CU)
__global__ void __launch_bounds__(64 * WGM * WGN, (SEG && BM == 64) ? ((PREC & kPrecBlockShift) ? 4 : 5) : (BM == 64 && BN == 128) ? 4 : 1)
conv_igemm(const ConvParams p) {
  constexpr bool BSHIFT = (PREC & kPrecBlockShift) != 0;
  constexpr bool POSM = (PREC & kPrecPosMajor) != 0;
  constexpr int PMODE = PREC & ~(kPrecBlockShift | kPrecPosMajor);   // the arithmetic (ConvPrec)
  static_assert(!POSM || (SEG && KS == 3 && BM == 64 && BN == 64 && !SHIFT && !RES && !DUAL && !BSHIFT && PMODE == kPrecF32),
                "position-major rows: the segmented fp32 3x3 on 64x64 tiles only (pos_major_valid)");
  static_assert(!BSHIFT || (!SHIFT && !RES), "block placement: a shifted identity (DUAL = false) or a shifted second source");
  constexpr bool RESID = RES || (BSHIFT && !DUAL);   // a residual is added (block placement: through the shift)
  static_assert(!SEG || (PMODE == kPrecF32 && !RES && WGM * WGN <= 4 && BM == BN && BM <= 64),
                "segmented K accumulation: fp32, 64x64 / 32x32 tiles, no residual (ConvParams::kseg_len)");
  static_assert(WGM * WGN == 4 || WGM * WGN == 1 || WGM * WGN == 8,
                "4 waves per workgroup, 1 (32x32 small-M tiles) or 8 (128x128 with 4 waves per SIMD at 2 workgroups/CU)");
  constexpr int NT = 64 * WGM * WGN;   // threads per workgroup
  constexpr int LRP = NT / 8;          // loader rows per pass (8 threads x 16 bytes per 128-byte row)
  static_assert(!DUAL || (KS == 1 && !SHIFT && !RES), "K-concatenated second source: plain 1x1 convs only");
  constexpr bool X3 = PMODE == kPrecBf16x3;
  constexpr bool BF = PMODE == kPrecBf16;   // plain bf16 storage, one bf16 MFMA per product (config 5)
  constexpr int EB = BF ? 2 : 4;           // bytes per stored element
  constexpr int KC = 128 / EB;             // channels per K-step (an LDS row is always 128 bytes)
  // (a shifted 3x3 holds two more offsets per pass; its segmented form is not built: ConvParams::kseg_len must be 0)
  static_assert(!SHIFT || KS == 1 || (KS == 3 && !SEG), "the temporal shift is fused into 1x1 and unsegmented 3x3 convs only");
  constexpr int WTM = BM / WGM, WTN = BN / WGN;
  constexpr int TM = WTM / 32, TN = WTN / 32;
  constexpr int APASS = BM / LRP, BPASS = BN / LRP;
  // RK ("register-resident K-step", fp32 64x64 / 32x32 tiles): ONE LDS buffer; after the barrier that makes a
  // tile visible every wave pulls all four k-groups of fragments into registers, a second barrier frees the
  // buffer, and the 16 MFMAs of the step then run from registers while the next tile is written into LDS.
  // Half the LDS per workgroup -> more workgroups per CU, and no LDS wait inside the MFMA sequence.
  constexpr bool RK = PMODE == kPrecF32 && ((BM == 64 && BN == 64) || (BM == 32 && BN == 32));
  // RK2 (fp32 64x128 tiles, unsegmented 1x1 only): the same step with a 32x64 wave tile -- one A and two B fragment sets per
  // k-group, 32 MFMAs on two independent accumulators, six loader items.  192 operand rows staged per 128 wave-MFMAs (64x64:
  // 128 per 64) and 12 fragment vectors read per 32 MFMAs (8 per 16): a quarter fewer operand bytes per MFMA on both paths.
  constexpr bool RK2 = PMODE == kPrecF32 && BM == 64 && BN == 128;
  static_assert(!RK2 || (WGM == 2 && WGN == 2 && KS == 1 && !SEG && !BSHIFT && !POSM),
                "64x128 tiles: unsegmented fp32 1x1 convs on 2x2 waves, no block placement (conv_tile_valid)");
  constexpr int NBUF = (RK || RK2) ? 1 : 2;
  constexpr int CLD = RK2 ? 68 : BN + 4;  // epilogue staging row stride (floats; 64x128 stages one 64-column half at a time)
  static_assert(TM >= 1 && TN >= 1, "wave tile must hold at least one 32x32 MFMA tile");
  constexpr int SMEM_FLOATS = NBUF * (BM + BN) * kLds > BM * CLD ? NBUF * (BM + BN) * kLds : BM * CLD;

  __shared__ __attribute__((aligned(16))) float smem[SMEM_FLOATS];

  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = tid >> 6;
  const int wm = wave / WGN, wn = wave % WGN;
  const int half = lane >> 5, l31 = lane & 31;

  // XCD-aware bijective remap: blocks b and b+8 share an XCD (and its L2); give each XCD a
  // contiguous run of tiles, n fastest, so co-resident blocks re-use the same A panel from L2.
  const int bid = blockIdx.x;
  const bool tail_mode = SEG && p.ksplit == 2;            // whole tiles first, then (tile, segment) pieces of the last rows of tiles
  // POSM with live-balanced runs (ConvParams::pos_whole > 0, pos_balanced_runs): XCD x owns the whole tiles pos_run[x] ..
  // pos_run[x + 1], the whole part of the grid is pos_whole = 8 x the longest run, and the tail's pieces follow THAT.
  bool balanced = false;
  if constexpr (POSM) balanced = p.pos_whole > 0;
  const int whole = balanced ? p.pos_whole : p.tail_from;   // tail mode: the workgroups in front of the pieces
  const bool in_tail = tail_mode && bid >= whole;
  const int nwg = tail_mode ? p.tail_from : balanced ? p.ntm * p.ntn : (int)gridDim.x;   // (the remap covers the whole tiles; the pieces go round-robin over the XCDs)
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  bool mirror = p.reverse != 0;   // walk the tiles from the far end (ConvParams::reverse)
  if constexpr (POSM) {
    if (balanced && !in_tail) {
      // A reverse walk gives XCD x run 7 - x from its end: the mirror image of the forward walk as a whole, and each XCD still
      // holds one balanced run (the mirror image of its own run need not be one: a tail split or stride 2 make the costs lopsided).
      const int run = p.reverse ? 7 - xcd : xcd, first = p.pos_run[run], len = p.pos_run[run + 1] - first, idx = bid >> 3;
      if (idx >= len) return;   // past this XCD's run: before any load or barrier, the whole workgroup alike
      tile = p.reverse ? first + len - 1 - idx : first + idx;
      mirror = false;
    }
  }
  if (mirror) tile = nwg - 1 - tile;
  int seg = 0;  // SEG + ksplit = 1: the grid holds ntm * ntn tiles per K segment, segment-major
  if (SEG && p.ksplit == 1) {
    seg = tile / (p.ntm * p.ntn);
    tile -= seg * (p.ntm * p.ntn);
  }
  if (in_tail) {
    const int u = bid - whole, n_tail = p.ntm * p.ntn - p.tail_from;
    seg = u / n_tail;
    tile = p.tail_from + (u - seg * n_tail);
  }
  const bool split_wg = SEG && (p.ksplit == 1 || in_tail);   // this workgroup multiplies ONE K segment and writes raw sums
  const int tm = tile / p.ntn, tn = tile - tm * p.ntn;
  const int m0 = tm * BM, n0 = tn * BN;

  // ---- descriptors, rebased to this workgroup's first input frame / first weight row ------------
  const int HoWo = p.Ho * p.Wo;
  const int n_first = POSM ? 0 : m0 / HoWo;   // (position-major: a tile's rows are 64 frames anywhere in the batch)
  const int frame0 = SHIFT ? (n_first > 0 ? n_first - 1 : 0) : n_first;
  // bf16-format stem: the input is stored as pixel PAIRS (8-element groups = 2 pixels x 4 channels, odd
  // widths padded with a zero pixel), so a frame is Hi x ceil(Wi/2) groups.
  constexpr bool PAIRS = KS == 7 && PMODE != kPrecF32;
  const int wpairs = (p.Wi + 1) >> 1;
  const size_t frame_elems = PAIRS ? (size_t)p.Hi * wpairs * 8 : (size_t)p.Hi * p.Wi * p.C;
  const size_t a_bytes = ((size_t)p.N - frame0) * frame_elems * EB;
  const __amdgpu_buffer_rsrc_t rsrcA = buffer_window(reinterpret_cast<const char *>(p.x) + (size_t)frame0 * frame_elems * EB, a_bytes);
  const __amdgpu_buffer_rsrc_t rsrcB = buffer_fixed(reinterpret_cast<const char *>(p.w) + (size_t)n0 * p.Kp * EB, BN * p.Kp * EB);

  // second A source (DUAL): same output pixels, its own channel count / spatial size / stride
  const size_t frame_elems2 = DUAL ? (size_t)p.Hi2 * p.Wi2 * p.C2 : 0;
  const int frame02 = (BSHIFT && DUAL && n_first > 0) ? n_first - 1 : n_first;   // (a shifted x2 also reads frame t-1)
  const size_t a2_bytes = DUAL ? ((size_t)p.N - frame02) * frame_elems2 * EB : 0;
  const __amdgpu_buffer_rsrc_t rsrcA2 = buffer_window(reinterpret_cast<const char *>(DUAL ? p.x2 : p.x) + (size_t)frame02 * frame_elems2 * EB, a2_bytes);

  // ---- per-thread loader state: 8 threads per 32-float row, 32 rows per pass -------------------
  const int lrow = tid >> 3;
  const int chunk = tid & 7;
  const int frame_bytes = (int)(frame_elems * EB);
  unsigned a_off[APASS];                       // byte offset of (row, tap 0, this thread's chunk)
  unsigned a_offp[SHIFT ? APASS : 1], a_offm[SHIFT ? APASS : 1];
  unsigned a_mask[(KS == 3 && !POSM) ? APASS : 1];
  // POSM: the tile's output position, its first frame and its live taps, all wave-uniform
  int pm_pos = 0, pm_n0 = 0;
  unsigned pm_live = 0x1ffu;
  if constexpr (POSM) {
    pos_major_row(m0, p.N, &pm_n0, &pm_pos);
    pm_live = pos_major_tap_mask(pm_pos, p.Wo, p.Hi, p.Wi, p.stride, p.pad);
  }
  unsigned a_off2[DUAL ? APASS : 1];
  unsigned a_off2p[(BSHIFT && DUAL) ? APASS : 1], a_off2m[(BSHIFT && DUAL) ? APASS : 1];
  int a_iy[KS == 7 ? APASS : 1], a_ix[KS == 7 ? APASS : 1];
#pragma unroll
  for (int pp = 0; pp < APASS; ++pp) {
    const int m = m0 + lrow + LRP * pp;
    const bool ok = POSM || m < p.M;   // (position-major: M % 64 == 0)
    const int mm = ok ? m : m0;
    const int n = POSM ? pm_n0 + lrow + LRP * pp : mm / HoWo;
    const int rem = POSM ? pm_pos : mm - n * HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
    if (KS == 7) {
      a_off[pp] = ok ? (unsigned)((n - frame0) * frame_bytes) : kInvalid;
      a_iy[pp] = iy0;
      // PAIRS: the 7 taps of a row (pixels 2ox-3 .. 2ox+3) sit in the 4 aligned pixel pairs starting at
      // pair ox-2 (pixel 2ox-4, whose weight is zero)
      a_ix[pp] = PAIRS ? (ix0 - 1) >> 1 : ix0;
    } else {
      const int base = (n - frame0) * frame_bytes + (iy0 * p.Wi + ix0) * p.C * EB + chunk * 16;
      a_off[pp] = (KS == 1 && !ok) ? kInvalid : (unsigned)base;
      if (DUAL)
        a_off2[pp] = ok ? (unsigned)((n - frame02) * (int)(frame_elems2 * EB) +
                                     (oy * p.stride2 * p.Wi2 + ox * p.stride2) * p.C2 * EB + chunk * 16)
                        : kInvalid;
      if (BSHIFT && DUAL) {   // x2's frames t+1 / t-1 (zeros past the clip's ends), chosen per chunk like the shifted A loader's
        const int t = n % p.T;
        a_off2p[pp] = (ok && t < p.T - 1) ? a_off2[pp] + (unsigned)(frame_elems2 * EB) : kInvalid;
        a_off2m[pp] = (ok && t > 0) ? a_off2[pp] - (unsigned)(frame_elems2 * EB) : kInvalid;
      }
      if (KS == 3 && !POSM) {
        unsigned mask = 0;
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
          for (int kx = 0; kx < 3; ++kx)
            if ((unsigned)(iy0 + ky) < (unsigned)p.Hi && (unsigned)(ix0 + kx) < (unsigned)p.Wi)
              mask |= 1u << (ky * 3 + kx);
        a_mask[pp] = ok ? mask : 0u;
      }
      if (SHIFT) {
        // channels [0,fold) <- frame t+1, [fold,2fold) <- frame t-1 (3x3: the same frame offset for every tap; the
        // tap's padding mask above still applies, a frame past the clip end reads zeros through kInvalid)
        const int t = n % p.T;
        a_offp[pp] = (ok && t < p.T - 1) ? (unsigned)(base + frame_bytes) : kInvalid;
        a_offm[pp] = (ok && t > 0) ? (unsigned)(base - frame_bytes) : kInvalid;
      }
    }
  }
  unsigned b_off[BPASS];
#pragma unroll
  for (int pp = 0; pp < BPASS; ++pp) b_off[pp] = (unsigned)((lrow + LRP * pp) * p.Kp * EB + chunk * 16);

  f32x4 ra[APASS], rb[BPASS];
  const int nk1 = DUAL ? p.K1 / KC : 0;

  // Loader work is cut into NITEMS = APASS + BPASS single-instruction items (one 16-B buffer load or
  // one ds_write_b128 each) so the main loop can drop one item between consecutive MFMAs.
  // A dead K-step (past the end of K) ORs kInvalid into every offset, so its loads return zeros
  // without touching memory and the loop body stays branch-free.
  constexpr int NITEMS = APASS + BPASS;
  struct KStep {  // wave-uniform per-K-step scalars
    unsigned kbytes;
    int tap, tap_off;
    unsigned dead;  // 0 for a live step, kInvalid for a step past the end of K (pure arithmetic, no select)
    unsigned mp, mm, m0;  // SHIFT: lane masks choosing the t+1 / t-1 / t source frame for this thread's chunk
  };
  auto kstep = [&](int kt, int nk_) {
    KStep k;
    k.kbytes = (unsigned)kt * (kBK * 4);
    k.dead = (~(unsigned)((kt - nk_) >> 31)) & kInvalid;
    k.tap = 0;
    k.tap_off = 0;
    int c0 = kt * KC;  // first input channel of this K-step
    if (KS == 3) {  // C >= 32 so a K-step never straddles a tap: tap and its offset are scalars
      k.tap = (kt * KC) >> (p.logC4 + 2);
      c0 = kt * KC - k.tap * p.C;
      const int ky = k.tap / 3, kx = k.tap - ky * 3;
      k.tap_off = ((ky * p.Wi + kx) * p.C + c0) * EB;
    }
    k.mp = k.mm = 0u;
    k.m0 = ~0u;
    if (SHIFT) {
      // channels [0,fold) <- frame t+1, [fold,2fold) <- frame t-1, rest <- frame t.  Kept as AND/OR
      // masks: a three-way select over the per-row offset arrays is turned into a scratch-memory
      // table by the compiler, which serialises the loader behind vmcnt(0).  fold % 4 (fp32) / % 8 (bf16
      // formats) keeps a 16-B chunk inside one group; a 3x3 K-step is (tap, channels c0 ..), same choice per tap.
      const int c = c0 + (X3 ? (chunk >> 1) * 8 : (BF ? chunk * 8 : chunk * 4));
      k.mp = 0u - (unsigned)(c < p.fold);
      k.mm = (0u - (unsigned)(c < 2 * p.fold)) & ~k.mp;
      k.m0 = ~(k.mp | k.mm);
    }
    if (BSHIFT && DUAL) {   // the same masks for a K-step of the second source (channel c0 - K1 of x2; unused on the first)
      const int c = c0 - nk1 * KC + (X3 ? (chunk >> 1) * 8 : (BF ? chunk * 8 : chunk * 4));
      k.mp = 0u - (unsigned)(c < p.fold);
      k.mm = (0u - (unsigned)(c < 2 * p.fold)) & ~k.mp;
      k.m0 = ~(k.mp | k.mm);
    }
    return k;
  };
  auto gload_item = [&](const KStep &k, int kt, int item) {
    if (item < APASS) {
      const int pp = item;
      if (KS == 1) {
        unsigned off = a_off[pp];
        if (SHIFT) off = (a_offp[pp] & k.mp) | (a_offm[pp] & k.mm) | (a_off[pp] & k.m0);
        if (DUAL) {
          // K-steps [0, nk1) come from the first source, the rest from the second (wave-uniform choice)
          const bool second = kt >= nk1;
          const unsigned off2 = BSHIFT ? (a_off2p[pp] & k.mp) | (a_off2m[pp] & k.mm) | (a_off2[pp] & k.m0) : a_off2[pp];
          ra[pp] = buf_load4(second ? rsrcA2 : rsrcA, (second ? off2 : off) | k.dead,
                             second ? k.kbytes - (unsigned)nk1 * 128u : k.kbytes);
        } else {
          ra[pp] = buf_load4(rsrcA, off | k.dead, k.kbytes);
        }
      } else if (KS == 3) {
        if (SHIFT) {
          // source frame of this chunk, then the tap; a zero frame (clip end) stays kInvalid instead of being offset
          const unsigned off = (a_offp[pp] & k.mp) | (a_offm[pp] & k.mm) | (a_off[pp] & k.m0);
          const bool ok = ((a_mask[pp] >> k.tap) & 1u) && off != kInvalid;
          ra[pp] = buf_load4(rsrcA, (ok ? off + (unsigned)k.tap_off : kInvalid) | k.dead, 0);
        } else if (POSM) {   // only live taps are walked
          ra[pp] = buf_load4(rsrcA, (a_off[pp] + (unsigned)k.tap_off) | k.dead, 0);
        } else {
          ra[pp] = buf_load4(rsrcA, (((a_mask[pp] >> k.tap) & 1u) ? a_off[pp] + (unsigned)k.tap_off : kInvalid) | k.dead, 0);
        }
      } else {
        if constexpr (PAIRS) {
          // bf16-format stem: K = (ky, pair j, pixel-in-pair, c4) = 7 x 4 x 8 = 224; one 8-element group
          // per 16-B chunk (bf16) or per chunk pair hi/lo (split); groups >= 28 are K padding
          const int g = X3 ? (kt * 8 + chunk) >> 1 : kt * 8 + chunk;
          const int ky = g >> 2, j = g & 3;
          const int iy = a_iy[pp] + ky, pc = a_ix[pp] + j;
          const bool ok = g < 28 && (unsigned)iy < (unsigned)p.Hi && (unsigned)pc < (unsigned)wpairs;
          const unsigned pix = X3 ? (unsigned)((iy * wpairs + pc) * 32 + (chunk & 1) * 16)
                                  : (unsigned)((iy * wpairs + pc) * 16);
          ra[pp] = buf_load4(rsrcA, (ok ? a_off[pp] + pix : kInvalid) | k.dead, 0);
        } else {
          // fp32 stem: C = 4 -> one tap per 16-B chunk; taps >= 49 are K padding
          const int tap = kt * 8 + chunk;
          const int ky = tap / 7, kx = tap - ky * 7;
          const int iy = a_iy[pp] + ky, ix = a_ix[pp] + kx;
          const bool ok = tap < 49 && (unsigned)iy < (unsigned)p.Hi && (unsigned)ix < (unsigned)p.Wi;
          ra[pp] = buf_load4(rsrcA, (ok ? a_off[pp] + (unsigned)((iy * p.Wi + ix) * 16) : kInvalid) | k.dead, 0);
        }
      }
    } else {
      const int pp = item - APASS;
      rb[pp] = buf_load4(rsrcB, b_off[pp] | k.dead, k.kbytes);
    }
  };
  auto lstore_item = [&](int buf, int item) {
    float *As = smem + buf * (BM + BN) * kLds;
    if (item < APASS)
      *reinterpret_cast<f32x4 *>(As + (lrow + LRP * item) * kLds + chunk * 4) = ra[item];
    else
      *reinterpret_cast<f32x4 *>(As + BM * kLds + (lrow + LRP * (item - APASS)) * kLds + chunk * 4) = rb[item - APASS];
  };

  f32x16 acc[TM][TN];
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // Fragment registers are double-buffered across the four 8-deep k-groups of a K-step so that the
  // LDS latency of group kk+1 hides under the 16 MFMAs (1024 cycles) of group kk.
  f32x4 af[2][TM], bf[2][TN];
  auto frag_load = [&](int buf, int kk, int set) {
    const float *As = smem + buf * (BM + BN) * kLds + (wm * WTM + l31) * kLds + half * 4;
    const float *Bs = smem + buf * (BM + BN) * kLds + BM * kLds + (wn * WTN + l31) * kLds + half * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) af[set][i] = *reinterpret_cast<const f32x4 *>(As + i * 32 * kLds + kk * 8);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf[set][j] = *reinterpret_cast<const f32x4 *>(Bs + j * 32 * kLds + kk * 8);
  };
  // 4*TM*TN MFMAs of one k-group; `inject(item)` is called NITEMS times, spread evenly between them,
  // and a scheduling fence pins each injected instruction behind the MFMA it follows: the matrix
  // pipe executes an issued MFMA for 64 cycles, during which the wave may issue the injected item.
  constexpr int NMFMA = 4 * TM * TN;
  auto mfma_group = [&](int set, auto &&inject) {
    int cnt = 0;
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[set][i][s], bf[set][j][s], acc[i][j], 0, 0, 0);
          ++cnt;
          const int done = (cnt * NITEMS) / NMFMA, before = ((cnt - 1) * NITEMS) / NMFMA;
#pragma unroll
          for (int it = before; it < done; ++it) {
            inject(it);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
  };
  auto no_inject = [](int) {};
  auto mfma_plain = [&](int set) {
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[set][i][s], bf[set][j][s], acc[i][j], 0, 0, 0);
  };
  (void)no_inject;

  // ---- split-bf16 fragments: an LDS row is 4 channel groups of [hi x8 | lo x8]; v_mfma_f32_32x32x16_bf16
  // takes A[row][k = 8*(lane>>5) + j], so k16-group q reads channel group g = 2q + (lane>>5).
  u32x4 ah[2][TM], al[2][TM], bh[2][TN], bl[2][TN];
  auto frag_load_x3 = [&](int buf, int qg, int set) {
    const float *As = smem + buf * (BM + BN) * kLds + (wm * WTM + l31) * kLds + (2 * qg + half) * 8;
    const float *Bs = smem + buf * (BM + BN) * kLds + BM * kLds + (wn * WTN + l31) * kLds + (2 * qg + half) * 8;
#pragma unroll
    for (int i = 0; i < TM; ++i) {
      ah[set][i] = *reinterpret_cast<const u32x4 *>(As + i * 32 * kLds);
      al[set][i] = *reinterpret_cast<const u32x4 *>(As + i * 32 * kLds + 4);
    }
#pragma unroll
    for (int j = 0; j < TN; ++j) {
      bh[set][j] = *reinterpret_cast<const u32x4 *>(Bs + j * 32 * kLds);
      bl[set][j] = *reinterpret_cast<const u32x4 *>(Bs + j * 32 * kLds + 4);
    }
  };
  constexpr int NMFMA3 = 3 * TM * TN;
  auto mfma_x3 = [&](int set, int nitems, auto &&inject) {
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int t = 0; t < 3; ++t) {
          const bf16x8 a = __builtin_bit_cast(bf16x8, t == 2 ? al[set][i] : ah[set][i]);
          const bf16x8 b = __builtin_bit_cast(bf16x8, t == 1 ? bl[set][j] : bh[set][j]);
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc[i][j], 0, 0, 0);
          ++cnt;
          const int done = (cnt * nitems) / NMFMA3, before = ((cnt - 1) * nitems) / NMFMA3;
#pragma unroll
          for (int it = before; it < done; ++it) {
            inject(it);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
  };

  // ---- plain bf16: a 128-byte LDS row is 64 channels = four k16-groups; group q, lane half h reads the 8
  // channels 16q + 8h (one ds_read_b128 per operand tile per MFMA).
  u32x4 af16[4][TM], bf16f[4][TN];
  auto frag_load_bf = [&](int buf, int qg) {
    const float *As = smem + buf * (BM + BN) * kLds + (wm * WTM + l31) * kLds + qg * 8 + half * 4;
    const float *Bs = smem + buf * (BM + BN) * kLds + BM * kLds + (wn * WTN + l31) * kLds + qg * 8 + half * 4;
#pragma unroll
    for (int i = 0; i < TM; ++i) af16[qg][i] = *reinterpret_cast<const u32x4 *>(As + i * 32 * kLds);
#pragma unroll
    for (int j = 0; j < TN; ++j) bf16f[qg][j] = *reinterpret_cast<const u32x4 *>(Bs + j * 32 * kLds);
  };
  constexpr int NMFMA_BF = TM * TN;
  auto mfma_bf = [&](int qg, int item0, int nitems, auto &&inject) {
    int cnt = 0;
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j) {
        acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af16[qg][i]),
                                                            __builtin_bit_cast(bf16x8, bf16f[qg][j]), acc[i][j], 0, 0, 0);
        ++cnt;
        const int done = (cnt * nitems) / NMFMA_BF, before = ((cnt - 1) * nitems) / NMFMA_BF;
#pragma unroll
        for (int it = before; it < done; ++it) {
          inject(item0 + it);
          __builtin_amdgcn_sched_barrier(0);
        }
      }
  };

  // Residual tile: fetched before the K loop (it does not depend on it) in the epilogue's own
  // row-major 16-B mapping, so its HBM latency hides under the MFMAs.  Rows past M read as zeros.
  constexpr int EW = (X3 || BF) ? 8 : 4;  // channels per thread per pass (split: one 32-byte group; bf16: 16 bytes)
  constexpr int TPR = BN / EW;         // threads per output row
  constexpr int RPP = NT / TPR;        // rows per pass
  constexpr int EPASS = BM / RPP;
  const int ecol = (tid % TPR) * EW, erow = tid / TPR;
  f32x4 rres[(RESID && !X3 && !BF && !RK2) ? EPASS : 1];   // (64x128: fetched under the last K-step, into the loader's registers)
  u32x4 rres_h[(RESID && (X3 || BF)) ? EPASS : 1], rres_l[(RESID && X3) ? EPASS : 1];
  if (RESID && (X3 || BF) && !BSHIFT) {
    const size_t r_bytes = ((size_t)p.M - m0) * p.Cout * EB;
    const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(reinterpret_cast<const char *>(p.res) + (size_t)m0 * p.Cout * EB, r_bytes);
#pragma unroll
    for (int k = 0; k < EPASS; ++k) {
      const unsigned o = (unsigned)(((erow + k * RPP) * p.Cout + n0 + ecol) * EB);
      rres_h[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (int)o, 0, 0);
      if (X3) rres_l[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (int)(o + 16), 0, 0);
    }
  }
  if (RESID && !X3 && !BF && !BSHIFT && !RK2) {
    const size_t r_bytes = ((size_t)p.M - m0) * p.Cout * 4;
    const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(p.res + (size_t)m0 * p.Cout, r_bytes);
#pragma unroll
    for (int k = 0; k < EPASS; ++k)
      rres[k] = buf_load4(rsrcR, (unsigned)(((erow + k * RPP) * p.Cout + n0 + ecol) * 4), 0);
  }
  if constexpr (RESID && BSHIFT) {
    // Block placement: the identity is the block input through the shift.  A thread's EW channels sit in one group (fold
    // % 4 / % 8), so its source row is row + Ho*Wo (channels [0, fold); zeros at the clip's last frame), row - Ho*Wo ([fold,
    // 2 fold); zeros at its first frame) or the row itself.  The descriptor starts one frame before the tile.
    const int rbase = m0 >= HoWo ? m0 - HoWo : 0;
    const int c = n0 + ecol;
    const int sel = c < p.fold ? 1 : c < 2 * p.fold ? -1 : 0;
    const unsigned step = (unsigned)(HoWo * p.Cout * EB);
    const size_t r_bytes = ((size_t)p.M - rbase) * p.Cout * EB;
    const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(reinterpret_cast<const char *>(p.res) + (size_t)rbase * p.Cout * EB, r_bytes);
#pragma unroll
    for (int k = 0; k < EPASS; ++k) {
      const int rr = erow + k * RPP;
      const int t = ((m0 + rr) / HoWo) % p.T;
      unsigned o = (unsigned)(((m0 - rbase + rr) * p.Cout + c) * EB);
      if (sel > 0) o = t < p.T - 1 ? o + step : kInvalid;
      if (sel < 0) o = t > 0 ? o - step : kInvalid;
      if constexpr (X3 || BF) {
        rres_h[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (int)o, 0, 0);
        if (X3) rres_l[k] = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (int)(o + 16), 0, 0);
      } else {
        rres[k] = buf_load4(rsrcR, o, 0);
      }
    }
  }

  // ---- main loop -------------------------------------------------------------------------------
  // Two LDS buffers, one barrier per K-step.  Iteration kt multiplies tile kt out of buf[kt&1] in four
  // k-groups of 4*TM*TN MFMAs:
  //   group 0            plain
  //   group 1            + ds_writes of tile kt+1 (registers, loaded during iteration kt-1) into the
  //                        other buffer: its last readers finished before the barrier of kt-1
  //   group 2            + buffer loads of tile kt+2, which then have a whole K-step to land
  //   barrier
  //   group 3            register-only, issued AFTER the barrier so that it covers the LDS latency of
  //                        the next tile's first fragments (read right after the barrier)
  // One barrier per step suffices: tile kt+1 is complete in LDS before it, and nobody overwrites
  // buf[kt&1] before the next barrier.  The body is straight-line.
  // This workgroup multiplies K-steps [kt0, nk): all of K, or one segment of it (SEG + ksplit).
  int kt0 = 0, nk = p.Kp / KC;
  if (split_wg) {
    kt0 = seg * p.kseg_len;
    nk = kt0 + p.kseg_len < nk ? kt0 + p.kseg_len : nk;
  }
  // SEG: `acc` holds the running segment, `tot` the sum of the finished ones (segment boundaries sit at
  // multiples of kseg_len from K-step 0 in both launch forms; kt0 is such a multiple).
  f32x16 tot[SEG ? TM : 1][SEG ? TN : 1];
  if constexpr (SEG) {
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
      for (int j = 0; j < TN; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) tot[i][j][e] = 0.f;
  }
  auto seg_flush = [&]() {
    if constexpr (SEG) {
#pragma unroll
      for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
          tot[i][j] += acc[i][j];
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
    }
  };
  // SEG loops are nested: the inner loop runs the K-steps of one segment, the flush sits between segments (kept
  // out of the inner loop on purpose: inside it the compiler if-converts the flush and drains the MFMA chain on
  // every K-step).  Without SEG there is a single pass over [kt0, nk).
  const int seg_len = (SEG && p.kseg_len > 0) ? p.kseg_len : 0x3fffffff;
  // POSM: the K-steps walked are the live taps' (pm_first, then next_live_kstep from one to the next; nk = none left, a dead step)
  const int pm_spt = POSM ? p.C / KC : 1;
  const int pm_first = POSM ? next_live_kstep(kt0, pm_live, pm_spt, nk) : kt0;
  const int pm_second = POSM ? next_live_kstep(pm_first + 1, pm_live, pm_spt, nk) : kt0 + 1;
  {
    const KStep k0 = kstep(pm_first, nk);
#pragma unroll
    for (int it = 0; it < NITEMS; ++it) gload_item(k0, pm_first, it);
#pragma unroll
    for (int it = 0; it < NITEMS; ++it) lstore_item(0, it);
    const KStep k1 = kstep(pm_second, nk);
#pragma unroll
    for (int it = 0; it < NITEMS; ++it) gload_item(k1, pm_second, it);
  }
  __syncthreads();
  if constexpr (BF) {
    // plain bf16: four k16-groups of TM*TN MFMAs per K-step.  Groups 0-1 carry the ds_writes of tile kt+1
    // and the buffer loads of tile kt+2; groups 2-3 run after the barrier and cover the next fragments.
    frag_load_bf(0, 0);
    frag_load_bf(0, 1);
    for (int kt = kt0; kt < nk; ++kt) {
      const int cur = (kt - kt0) & 1;
      const KStep k2 = kstep(kt + 2, nk);
      frag_load_bf(cur, 2);
      frag_load_bf(cur, 3);
      auto inject = [&](int it) {
        if (it < NITEMS) lstore_item(cur ^ 1, it);
        else gload_item(k2, kt + 2, it - NITEMS);
      };
      mfma_bf(0, 0, NITEMS, inject);
      mfma_bf(1, NITEMS, NITEMS, inject);
      __syncthreads();
      __builtin_amdgcn_sched_barrier(0);
      mfma_bf(2, 0, 0, [](int) {});
      frag_load_bf(cur ^ 1, 0);
      __builtin_amdgcn_sched_barrier(0);
      mfma_bf(3, 0, 0, [](int) {});
      __builtin_amdgcn_sched_barrier(0);
      frag_load_bf(cur ^ 1, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  } else if constexpr (RK2) {
    // One step = fragments of all four k-groups (A: 4 vectors, B: 2 column tiles x 4), the barrier that frees the buffer, then
    // 32 MFMAs from registers: k-group ascending, s ascending, acc[0][0] then acc[0][1] -- each accumulator sees the 64x64
    // arm's sequence.  The 2 * NITEMS loader items (ds_writes of tile kt+1, then the loads of kt+2) go between the first 24.
    f32x4 fa[4], fb[2][4];
    auto frags = [&]() {
      const float *As = smem + (wm * WTM + l31) * kLds + half * 4;
      const float *Bs = smem + BM * kLds + (wn * WTN + l31) * kLds + half * 4;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk) {
        fa[kk] = *reinterpret_cast<const f32x4 *>(As + kk * 8);
#pragma unroll
        for (int j = 0; j < 2; ++j) fb[j][kk] = *reinterpret_cast<const f32x4 *>(Bs + j * 32 * kLds + kk * 8);
      }
    };
    auto mfma_step = [&](auto &&inject) {
      int cnt = 0;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4)
#pragma unroll
          for (int j = 0; j < 2; ++j) {
            acc[0][j] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa[kk][s4], fb[j][kk][s4], acc[0][j], 0, 0, 0);
            ++cnt;
            const int done = cnt < 24 ? (cnt * 2 * NITEMS) / 24 : 2 * NITEMS;
            const int before = cnt - 1 < 24 ? ((cnt - 1) * 2 * NITEMS) / 24 : 2 * NITEMS;
#pragma unroll
            for (int it = before; it < done; ++it) {
              inject(it);
              __builtin_amdgcn_sched_barrier(0);
            }
          }
    };
    for (int kt = kt0; kt < nk - 1; ++kt) {
      const KStep k2 = kstep(kt + 2, nk);
      frags();
      __syncthreads();  // every wave holds its fragments: the buffer may be overwritten
      mfma_step([&](int it) {
        if (it < NITEMS) lstore_item(0, it);
        else gload_item(k2, kt + 2, it - NITEMS);
      });
      __syncthreads();  // tile kt+1 is complete in LDS
    }
    // The last K-step has nothing to stage, so the loader's registers are free: the residual of the first 64-column half (four
    // vectors in the epilogue's mapping) is fetched here, under the step's MFMAs, and the second half's once the fragment
    // registers are free, under the first half's staging and stores.  All eight before the loop, as the other tiles fetch
    // theirs, do not fit the 128-register budget.
    frags();
    __syncthreads();  // the operand buffer is free: the epilogue stages into it
    // Epilogue mapping: 16 threads per row of a 64-column half, 16 rows per pass, 4 passes.  Half h holds column tile h of both
    // wave columns: staging column c is output column n0 + 64 * (c / 32) + 32 * h + c % 32, so all four waves stage and every
    // thread's 16 bytes stay inside one 128-byte run.
    const int hrow = tid >> 4, hcol = (tid & 15) * 4;
    const int ocol = n0 + (hcol >> 5) * 64 + (hcol & 31);
    f32x4 rr2[RES ? 2 : 1][RES ? 4 : 1];
    auto res_half = [&](int h) {
      if constexpr (RES) {
        const size_t r_bytes = ((size_t)p.M - m0) * p.Cout * 4;
        const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(p.res + (size_t)m0 * p.Cout, r_bytes);   // (rows past M read as zeros)
#pragma unroll
        for (int k = 0; k < 4; ++k) rr2[h][k] = buf_load4(rsrcR, (unsigned)(((hrow + 16 * k) * p.Cout + ocol + 32 * h) * 4), 0);
      }
    };
    res_half(0);
    mfma_step([](int) {});
    __builtin_amdgcn_sched_barrier(0);
    res_half(1);
    const size_t y_bytes = ((size_t)p.M - m0) * p.Cout * 4;   // rows past M are dropped by the range check
    const __amdgpu_buffer_rsrc_t rsrcY = buffer_window(reinterpret_cast<char *>(p.y) + (size_t)m0 * p.Cout * 4, y_bytes);
    const float floor_ = p.relu ? 0.f : -INFINITY;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if (h) __syncthreads();  // half 0 has been read out
#pragma unroll
      for (int e = 0; e < 16; ++e)
        smem[(wm * WTM + (e & 3) + 8 * (e >> 2) + 4 * half) * CLD + wn * 32 + l31] = acc[0][h][e];
      __syncthreads();
      const f32x4 bias = *reinterpret_cast<const f32x4 *>(p.bias + ocol + 32 * h);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const int rr = hrow + 16 * k;
        f32x4 v = *reinterpret_cast<const f32x4 *>(smem + rr * CLD + hcol);
        v += bias;
        if constexpr (RES) v += rr2[h][k];
        v[0] = fmaxf(v[0], floor_);
        v[1] = fmaxf(v[1], floor_);
        v[2] = fmaxf(v[2], floor_);
        v[3] = fmaxf(v[3], floor_);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrcY, (int)((rr * p.Cout + ocol + 32 * h) * 4), 0, 0);
      }
    }
    return;
  } else if constexpr (RK) {
    f32x4 ra_[4], rb_[4];  // all four k-groups of this wave's A / B fragments (TM = TN = 1)
    // fp32 stem: K = 49 taps x 4 channels = 196 of the 224 padded, so the last K-step holds real data in its first
    // 4 k only: it runs as a 4-MFMA tail instead of 16 (the 12 skipped MFMAs multiply zeros; same bits).
    const bool trim = KS == 7 && p.Kp == 224 && nk == 7;
    const int nk_full = trim ? nk - 1 : nk;
    if constexpr (POSM) {
      // The loop below over the live steps only: kt is the step in LDS, kt1 the one in the loader registers, kt2 the one whose
      // loads are injected.  A segment ends at its boundary in absolute K-steps, so the segment sums and their order are the
      // natural arm's; a segment without a live step is never entered (its flush would add +0).  The step's body is the
      // natural loop's, word for word (a lambda shared by both moved other instantiations' registers).
      int kt = pm_first, kt1 = pm_second;
      while (kt < nk) {
        const int bound = (kt / seg_len + 1) * seg_len, kend = bound < nk ? bound : nk;
        while (kt < kend) {
          const int kt2 = next_live_kstep(kt1 + 1, pm_live, pm_spt, nk);
          const KStep k2 = kstep(kt2, nk);
          {
            const float *As = smem + (wm * WTM + l31) * kLds + half * 4;
            const float *Bs = smem + BM * kLds + (wn * WTN + l31) * kLds + half * 4;
#pragma unroll
            for (int kk = 0; kk < 4; ++kk) {
              ra_[kk] = *reinterpret_cast<const f32x4 *>(As + kk * 8);
              rb_[kk] = *reinterpret_cast<const f32x4 *>(Bs + kk * 8);
            }
          }
          __syncthreads();  // every wave holds its fragments: the buffer may be overwritten
          int cnt = 0;
#pragma unroll
          for (int kk = 0; kk < 4; ++kk)
#pragma unroll
            for (int s4 = 0; s4 < 4; ++s4) {
              acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra_[kk][s4], rb_[kk][s4], acc[0][0], 0, 0, 0);
              ++cnt;
              // 2*NITEMS loader items over the first 12 MFMAs: the ds_writes of tile kt+1, then the loads of kt+2
              const int done = cnt < 12 ? (cnt * 2 * NITEMS) / 12 : 2 * NITEMS;
              const int before = cnt - 1 < 12 ? ((cnt - 1) * 2 * NITEMS) / 12 : 2 * NITEMS;
#pragma unroll
              for (int it = before; it < done; ++it) {
                if (it < NITEMS) lstore_item(0, it);
                else gload_item(k2, kt2, it - NITEMS);
                __builtin_amdgcn_sched_barrier(0);
              }
            }
          __syncthreads();  // tile kt+1 is complete in LDS
          kt = kt1;
          kt1 = kt2;
        }
        seg_flush();
      }
    } else {
    for (int kt = kt0; kt < nk_full;) {
    const int kend = (SEG && kt + seg_len < nk_full) ? kt + seg_len : nk_full;
    for (; kt < kend; ++kt) {
      const KStep k2 = kstep(kt + 2, nk);
      {
        const float *As = smem + (wm * WTM + l31) * kLds + half * 4;
        const float *Bs = smem + BM * kLds + (wn * WTN + l31) * kLds + half * 4;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk) {
          ra_[kk] = *reinterpret_cast<const f32x4 *>(As + kk * 8);
          rb_[kk] = *reinterpret_cast<const f32x4 *>(Bs + kk * 8);
        }
      }
      __syncthreads();  // every wave holds its fragments: the buffer may be overwritten
      int cnt = 0;
#pragma unroll
      for (int kk = 0; kk < 4; ++kk)
#pragma unroll
        for (int s4 = 0; s4 < 4; ++s4) {
          acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(ra_[kk][s4], rb_[kk][s4], acc[0][0], 0, 0, 0);
          ++cnt;
          // 2*NITEMS loader items over the first 12 MFMAs: the ds_writes of tile kt+1, then the loads of kt+2
          const int done = cnt < 12 ? (cnt * 2 * NITEMS) / 12 : 2 * NITEMS;
          const int before = cnt - 1 < 12 ? ((cnt - 1) * 2 * NITEMS) / 12 : 2 * NITEMS;
#pragma unroll
          for (int it = before; it < done; ++it) {
            if (it < NITEMS) lstore_item(0, it);
            else gload_item(k2, kt + 2, it - NITEMS);
            __builtin_amdgcn_sched_barrier(0);
          }
        }
      __syncthreads();  // tile kt+1 is complete in LDS
    }
    seg_flush();
    }
    }
    if (KS == 7 && trim) {
      const f32x4 a0 = *reinterpret_cast<const f32x4 *>(smem + (wm * WTM + l31) * kLds + half * 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4 *>(smem + BM * kLds + (wn * WTN + l31) * kLds + half * 4);
      __syncthreads();  // fragments are in registers: the epilogue may reuse the buffer
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4)
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s4], b0[s4], acc[0][0], 0, 0, 0);
    }
  } else if constexpr (!X3) {
    frag_load(0, 0, 0);
    frag_load(0, 1, 1);
    for (int kt = kt0; kt < nk;) {
    const int kend = (SEG && kt + seg_len < nk) ? kt + seg_len : nk;
    for (; kt < kend; ++kt) {
      const int cur = (kt - kt0) & 1;
      const KStep k2 = kstep(kt + 2, nk);
      mfma_plain(0);
      frag_load(cur, 2, 0);
      mfma_group(1, [&](int it) { lstore_item(cur ^ 1, it); });
      frag_load(cur, 3, 1);
      mfma_group(0, [&](int it) { gload_item(k2, kt + 2, it); });
      __syncthreads();
      frag_load(cur ^ 1, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      mfma_plain(1);
      __builtin_amdgcn_sched_barrier(0);
      frag_load(cur ^ 1, 1, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
    seg_flush();
    }
  } else {
    // split-bf16: a K-step is two k16-groups of 3*TM*TN MFMAs (32 cycles each).  Group 0 carries the
    // ds_writes of tile kt+1 and the buffer loads of tile kt+2; group 1 is issued after the barrier and
    // covers the LDS latency of the next tile's fragments.  Same buffer/barrier reasoning as above.
    frag_load_x3(0, 0, 0);
    frag_load_x3(0, 1, 1);
    for (int kt = kt0; kt < nk; ++kt) {
      const int cur = (kt - kt0) & 1;
      const KStep k2 = kstep(kt + 2, nk);
      mfma_x3(0, 2 * NITEMS, [&](int it) {
        if (it < NITEMS) lstore_item(cur ^ 1, it);
        else gload_item(k2, kt + 2, it - NITEMS);
      });
      __syncthreads();
      frag_load_x3(cur ^ 1, 0, 0);
      __builtin_amdgcn_sched_barrier(0);
      mfma_x3(1, 0, [](int) {});
      __builtin_amdgcn_sched_barrier(0);
      frag_load_x3(cur ^ 1, 1, 1);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  // ---- epilogue ---------------------------------------------------------------------------------
  // C/D layout: col = lane&31, row = (reg&3) + 8*(reg>>2) + 4*(lane>>5).  Stage the BM x BN tile in
  // LDS (all operand reads finished at the barrier above), then stream it out row-major.
  float *Cs = smem;  // (SEG: every segment, the last one included, was flushed into tot after its inner loop)
#pragma unroll
  for (int i = 0; i < TM; ++i)
#pragma unroll
    for (int j = 0; j < TN; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e)
        Cs[(wm * WTM + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * half) * CLD + wn * WTN + j * 32 + l31] =
            SEG ? tot[SEG ? i : 0][SEG ? j : 0][e] : acc[i][j][e];
  __syncthreads();

  // Stores go through a descriptor that ends at row M: rows past the end are dropped by the range
  // check, which keeps the epilogue branch-free (no per-pass wait on earlier stores).
  const bool partial = split_wg;  // raw segment sums to y = partial[seg][M][Cout] (tail split: ypart = partial[seg][tail rows][Cout]): no bias, no ReLU
  // POSM: a whole tile's row rr is frame pm_n0 + rr at position pm_pos, row (pm_n0 + rr) * HoWo + pm_pos of y (the descriptor
  // starts at p.y and spans it); a tail piece writes ypart in m' order like any other (the reduction maps its rows)
  const bool y_scatter = POSM && !in_tail;
  const size_t y_bytes = ((size_t)p.M - (y_scatter ? 0 : m0)) * p.Cout * EB;
  const int mt0 = in_tail ? (p.tail_from / p.ntn) * BM : 0;   // first row of the tail
  char *ybase = y_scatter ? reinterpret_cast<char *>(p.y) : in_tail ? reinterpret_cast<char *>(p.ypart) + ((size_t)seg * (p.M - mt0) + (m0 - mt0)) * p.Cout * EB
                        : reinterpret_cast<char *>(p.y) + ((size_t)(partial ? seg : 0) * p.M + m0) * p.Cout * EB;
  const __amdgpu_buffer_rsrc_t rsrcY = buffer_window(ybase, y_bytes);
  const float floor_ = (p.relu && !partial) ? 0.f : -INFINITY;  // ReLU as a branch-free clamp
  if constexpr (BF) {
    const f32x4 bias0 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + ecol);
    const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + ecol + 4);
#pragma unroll
    for (int k = 0; k < EPASS; ++k) {
      const int rr = erow + k * RPP;
      const f32x4 c0 = *reinterpret_cast<const f32x4 *>(Cs + rr * CLD + ecol);
      const f32x4 c1 = *reinterpret_cast<const f32x4 *>(Cs + rr * CLD + ecol + 4);
      float v[8] = {c0[0] + bias0[0], c0[1] + bias0[1], c0[2] + bias0[2], c0[3] + bias0[3],
                    c1[0] + bias1[0], c1[1] + bias1[1], c1[2] + bias1[2], c1[3] + bias1[3]};
      if (RESID) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += split_elem(rres_h[k], e);
      }
      u32x4 o;
#pragma unroll
      for (int w = 0; w < 4; ++w) o[w] = pack_bf16(fmaxf(v[2 * w], floor_), fmaxf(v[2 * w + 1], floor_));
      __builtin_amdgcn_raw_buffer_store_b128(o, rsrcY, (rr * p.Cout + n0 + ecol) * 2, 0, 0);
    }
  } else if constexpr (!X3) {
    f32x4 bias = *reinterpret_cast<const f32x4 *>(p.bias + n0 + ecol);
    if (partial) bias = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < EPASS; ++k) {
      const int rr = erow + k * RPP;
      f32x4 v = *reinterpret_cast<const f32x4 *>(Cs + rr * CLD + ecol);
      v += bias;
      if (RESID) v += rres[k];
      v[0] = fmaxf(v[0], floor_);
      v[1] = fmaxf(v[1], floor_);
      v[2] = fmaxf(v[2], floor_);
      v[3] = fmaxf(v[3], floor_);
      const int yr = y_scatter ? (pm_n0 + rr) * HoWo + pm_pos : rr;
      __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, v), rsrcY,
                                             (int)((yr * p.Cout + n0 + ecol) * 4), 0, 0);
    }
  } else {
    const f32x4 bias0 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + ecol);
    const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + ecol + 4);
#pragma unroll
    for (int k = 0; k < EPASS; ++k) {
      const int rr = erow + k * RPP;
      const f32x4 c0 = *reinterpret_cast<const f32x4 *>(Cs + rr * CLD + ecol);
      const f32x4 c1 = *reinterpret_cast<const f32x4 *>(Cs + rr * CLD + ecol + 4);
      float v[8] = {c0[0] + bias0[0], c0[1] + bias0[1], c0[2] + bias0[2], c0[3] + bias0[3],
                    c1[0] + bias1[0], c1[1] + bias1[1], c1[2] + bias1[2], c1[3] + bias1[3]};
      if (RESID) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += split_elem(rres_h[k], e) + split_elem(rres_l[k], e);
      }
      u32x4 oh, ol;
#pragma unroll
      for (int w = 0; w < 4; ++w) {
        const float x0 = fmaxf(v[2 * w], floor_), x1 = fmaxf(v[2 * w + 1], floor_);
        unsigned hw, lw;
        split_pair(x0, x1, &hw, &lw);
        oh[w] = hw;
        ol[w] = lw;
      }
      const int o = (rr * p.Cout + n0 + ecol) * 4;
      __builtin_amdgcn_raw_buffer_store_b128(oh, rsrcY, o, 0, 0);
      __builtin_amdgcn_raw_buffer_store_b128(ol, rsrcY, o + 16, 0, 0);
    }
  }
}

// Launch: conv_route (tsm_conv_rules.h) has decided everything; this maps a route to its instantiation.  The launch trace records a kernel as
// its launch line spells it, with the enclosing function's template arguments, and tests pin both: so every instantiation keeps a launch line,
// and the per-precision triple is a macro over the arm's spelling, not a template (whose line would read the same for every arm).
#define TSM_KLAUNCH_WALK_X(rev, kern, ...) TSM_KLAUNCH_WALK(rev, kern, __VA_ARGS__)   // (expands `kern` before it is spelled)
// ARM(PREC): an arm's instantiation for one precision (TSM_ARM_*: they spell BM .. RES of the enclosing template); launched for p.prec out
// of a function with p, grid, block, s, which then RETURNS the launch status.
#define TSM_LAUNCH_IGEMM_AND_RETURN(ARM)                                                                \
  do {                                                                                                  \
    if (p.prec == kPrecBf16x3) TSM_KLAUNCH_WALK_X(p.reverse, ARM(kPrecBf16x3), grid, block, 0, s, p);   \
    else if (p.prec == kPrecBf16) TSM_KLAUNCH_WALK_X(p.reverse, ARM(kPrecBf16), grid, block, 0, s, p);  \
    else TSM_KLAUNCH_WALK_X(p.reverse, ARM(kPrecF32), grid, block, 0, s, p);                            \
    return hipGetLastError();                                                                           \
  } while (0)
#define TSM_ARM_DUAL_SHIFT(PREC) (conv_igemm<BM, BN, WGM, WGN, 1, false, false, PREC | kPrecBlockShift, true>)
#define TSM_ARM_DUAL(PREC) (conv_igemm<BM, BN, WGM, WGN, 1, false, false, PREC, true>)
#define TSM_ARM_RES_SHIFT(PREC) (conv_igemm<BM, BN, WGM, WGN, KS, false, false, PREC | kPrecBlockShift>)
#define TSM_ARM_PLAIN(PREC) (conv_igemm<BM, BN, WGM, WGN, KS, SHIFT, RES, PREC>)

// Segmented-K instantiations (fp32, 64x64 / 32x32 tiles, no residual): one workgroup per tile, or per
// (tile, segment) when p.ksplit is set.
template <int BM, int BN, int WGM, int WGN, int KS, bool SHIFT>
static hipError_t launch_conv_seg(const ConvParams &p, const ConvRoute &r, hipStream_t s) {
  if constexpr (!((BM == 64 && BN == 64) || (BM == 32 && BN == 32))) {
    return hipErrorInvalidValue;
  } else {
    const dim3 grid(r.grid), block(64 * WGM * WGN);
    if constexpr (KS == 1 && !SHIFT) {
      if (r.dual) {   // (block_shift: block placement, the downsample operand through the shift)
        if (r.block_shift) TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<BM, BN, WGM, WGN, 1, false, false, kPrecF32 | kPrecBlockShift, true, true>), grid, block, 0, s, p);
        else TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<BM, BN, WGM, WGN, 1, false, false, kPrecF32, true, true>), grid, block, 0, s, p);
        return hipGetLastError();
      }
    }
    if constexpr (BM == 64 && WGM == 2 && KS == 3 && !SHIFT) {
      if (r.pos_major) {   // position-major rows (ConvParams::pos_major where pos_major_valid holds)
        // the trace line says when the launch runs live-balanced XCD runs, and on what grid: the route's, as the kernel gets it
        char mark[48];
        snprintf(mark, sizeof mark, " [balanced %d/%ld]", p.pos_whole, p.ksplit == 2 ? (long)p.tail_from : r.tiles);
        TSM_KLAUNCH_WALK_MARK(p.reverse, p.pos_whole > 0 ? mark : nullptr,
                              (conv_igemm<64, 64, 2, 2, 3, false, false, kPrecF32 | kPrecPosMajor, false, true>), grid, block, 0, s, p);
        return hipGetLastError();
      }
    }
    TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<BM, BN, WGM, WGN, KS, SHIFT, false, kPrecF32, false, true>), grid, block, 0, s, p);
    return hipGetLastError();
  }
}

template <int BM, int BN, int WGM, int WGN, int KS, bool SHIFT, bool RES>
static hipError_t launch_conv_t(const ConvParams &p, const ConvRoute &r, hipStream_t s) {
  if (r.family == kFamIgemmSeg) {
    if constexpr (!RES && KS != 7 && !(SHIFT && KS == 3)) return launch_conv_seg<BM, BN, WGM, WGN, KS, SHIFT>(p, r, s);
    else return hipErrorInvalidValue;
  }
  const dim3 grid(r.grid), block(64 * WGM * WGN);
  if constexpr (KS == 1 && !SHIFT && !RES) {
    if (r.dual && r.block_shift) TSM_LAUNCH_IGEMM_AND_RETURN(TSM_ARM_DUAL_SHIFT);   // block placement: the downsample operand through the shift
    if (r.dual) TSM_LAUNCH_IGEMM_AND_RETURN(TSM_ARM_DUAL);
  }
  if constexpr (RES && !SHIFT && KS != 7) {
    if (r.block_shift) TSM_LAUNCH_IGEMM_AND_RETURN(TSM_ARM_RES_SHIFT);              // block placement: the identity through the shift
  }
  TSM_LAUNCH_IGEMM_AND_RETURN(TSM_ARM_PLAIN);
}

// The 64x128 tile (kTile64x128; conv_route: fp32, unsegmented 1x1, no block placement): its four arms, one launch line each.
static hipError_t launch_conv_64x128(const ConvParams &p, const ConvRoute &r, hipStream_t s) {
  if (r.ks != 1 || r.family != kFamIgemm || r.block_shift || p.prec != kPrecF32) return hipErrorInvalidValue;
  const dim3 grid(r.grid), block(256);
  if (r.dual) TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<64, 128, 2, 2, 1, false, false, kPrecF32, true>), grid, block, 0, s, p);
  else if (r.res) TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<64, 128, 2, 2, 1, false, true, kPrecF32>), grid, block, 0, s, p);
  else if (r.shift) TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<64, 128, 2, 2, 1, true, false, kPrecF32>), grid, block, 0, s, p);
  else TSM_KLAUNCH_WALK(p.reverse, (conv_igemm<64, 128, 2, 2, 1, false, false, kPrecF32>), grid, block, 0, s, p);
  return hipGetLastError();
}

template <int KS, bool SHIFT, bool RES>
static hipError_t launch_conv_ks(const ConvParams &p, const ConvRoute &r, hipStream_t s) {
  if (r.bm == 32) return launch_conv_t<32, 32, 1, 1, KS, SHIFT, RES>(p, r, s);
  if (r.bm == 128 && r.bn == 128 && r.wgm == 4) return launch_conv_t<128, 128, 4, 2, KS, SHIFT, RES>(p, r, s);
  if (r.bm == 128 && r.bn == 128) return launch_conv_t<128, 128, 2, 2, KS, SHIFT, RES>(p, r, s);
  if (r.bm == 128) return launch_conv_t<128, 64, 2, 2, KS, SHIFT, RES>(p, r, s);
  return launch_conv_t<64, 64, 2, 2, KS, SHIFT, RES>(p, r, s);
}

hipError_t launch_conv(const ConvParams &p_in, int ks, hipStream_t s) {
  // These tile codes' families size a persistent grid by the device's CU count and need its > 64 KB LDS opt-in: asked BEFORE the
  // route, which takes the CU count (so a launch that its arguments refuse has run device_info() too).
  const bool device = p_in.tile == kTile256x256 || p_in.tile == kTile256x256p || p_in.tile == kTileWs;
  const DeviceInfo *di = device ? &device_info() : nullptr;
  const ConvRoute r = conv_route(p_in, ks, di ? di->n_cu : 0);
  if (r.family == kFamInvalid) return hipErrorInvalidValue;
  if (di && di->status != hipSuccess) return di->status;
  ConvParams p = p_in;
  p.ntm = r.ntm; p.ntn = r.ntn;
  p.pos_whole = r.pos_whole;   // (0 unless the route runs live-balanced position-major runs)
  for (int k = 0; k <= kXcds; ++k) p.pos_run[k] = r.pos_run[k];
  if (r.family == kFamBf16_256 || r.family == kFamBf16_256p) return launch_conv_bf16_256(p, r, s);
  if (r.family >= kFamWs3x3) return launch_conv_ws(p, r, s);
  if (p.ksplit == 2 && !p.ypart) return hipErrorInvalidValue;   // (the tail split's segment sums)
  if (r.bm == 64 && r.bn == 128) return launch_conv_64x128(p, r, s);
  if (ks == 1) return r.res ? launch_conv_ks<1, false, true>(p, r, s) : r.shift ? launch_conv_ks<1, true, false>(p, r, s) : launch_conv_ks<1, false, false>(p, r, s);
  if (ks == 3) return r.res ? launch_conv_ks<3, false, true>(p, r, s) : r.shift ? launch_conv_ks<3, true, false>(p, r, s) : launch_conv_ks<3, false, false>(p, r, s);
  return launch_conv_ks<7, false, false>(p, r, s);
}

// ---------------------------------------------------------------------------------------------
// Split-K reduction (fp32): the segment sums of a ksplit launch are added in segment order -- the order the
// unsplit kernel uses -- then bias, residual and ReLU exactly as in the conv epilogue.  4 channels per thread.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) splitk_reduce_kernel(const float *__restrict__ partial, int n_seg, int64_t n4,
                                                            int64_t seg_stride4, int cout4,
                                                            const float *__restrict__ bias, const float *__restrict__ res,
                                                            float *__restrict__ y, int relu) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float floor_ = relu ? 0.f : -INFINITY;
  const f32x4 *p4 = reinterpret_cast<const f32x4 *>(partial);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 t = p4[i];
    for (int sgm = 1; sgm < n_seg; ++sgm) t += p4[i + sgm * seg_stride4];
    f32x4 v = t + reinterpret_cast<const f32x4 *>(bias)[i % cout4];
    if (res) v += reinterpret_cast<const f32x4 *>(res)[i];
    v[0] = fmaxf(v[0], floor_);
    v[1] = fmaxf(v[1], floor_);
    v[2] = fmaxf(v[2], floor_);
    v[3] = fmaxf(v[3], floor_);
    reinterpret_cast<f32x4 *>(y)[i] = v;
  }
}


// The same for the tail of a position-major launch (ConvParams::pos_major): row i of the segment sums is GEMM row m_first + i,
// frame m' % n_frames at position m' / n_frames, and goes to row frame * howo + position of y (y: the whole output).
__global__ void __launch_bounds__(256) splitk_reduce_pos_kernel(const float *__restrict__ partial, int n_seg, int64_t n4,
                                                                int64_t seg_stride4, int cout4, int m_first, int n_frames,
                                                                int howo, const float *__restrict__ bias,
                                                                float *__restrict__ y, int relu) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  const float floor_ = relu ? 0.f : -INFINITY;
  const f32x4 *p4 = reinterpret_cast<const f32x4 *>(partial);
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
    f32x4 t = p4[i];
    for (int sgm = 1; sgm < n_seg; ++sgm) t += p4[i + sgm * seg_stride4];
    const int row = (int)(i / cout4), c4 = (int)(i - (int64_t)row * cout4);
    int frame, pos;
    pos_major_row(m_first + row, n_frames, &frame, &pos);
    f32x4 v = t + reinterpret_cast<const f32x4 *>(bias)[c4];
    v[0] = fmaxf(v[0], floor_);
    v[1] = fmaxf(v[1], floor_);
    v[2] = fmaxf(v[2], floor_);
    v[3] = fmaxf(v[3], floor_);
    reinterpret_cast<f32x4 *>(y)[((int64_t)frame * howo + pos) * cout4 + c4] = v;
  }
}

hipError_t launch_splitk_reduce_pos(const float *partial, int n_seg, int64_t m_first, int64_t m, int n_frames, int howo, int cout,
                                    const float *bias, float *y, int relu, hipStream_t s) {
  if (!partial || !bias || !y || n_seg < 1 || m_first < 0 || m <= 0 || n_frames <= 0 || howo <= 0 || cout <= 0 || cout % 4 != 0 ||
      m_first + m != (int64_t)n_frames * howo || (m_first + m) * cout >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  const int64_t n4 = m * cout / 4;
  TSM_KLAUNCH(splitk_reduce_pos_kernel, dim3(grid_for(n4, 2048)), dim3(256), 0, s, partial, n_seg, n4, n4, cout / 4, (int)m_first,
                     n_frames, howo, bias, y, relu);
  return hipGetLastError();
}

hipError_t launch_splitk_reduce(const float *partial, int n_seg, int64_t m, int cout, const float *bias,
                                const float *res, float *y, int relu, hipStream_t s) {
  if (!partial || !bias || !y || n_seg < 1 || m <= 0 || cout <= 0 || cout % 4 != 0) return hipErrorInvalidValue;
  const int64_t n4 = m * cout / 4;
  TSM_KLAUNCH(splitk_reduce_kernel, dim3(grid_for(n4, 2048)), dim3(256), 0, s, partial, n_seg, n4, n4, cout / 4,
                     bias, res, y, relu);
  return hipGetLastError();
}

}  // namespace tsm
