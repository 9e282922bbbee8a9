// conv_bf16_256[p]_kernel: the bf16 implicit GEMM on a 256 x 256 tile, operands by LDS-DMA (one-shot and persistent).
#include "tsm_device.h"

namespace tsm {

// ---------------------------------------------------------------------------------------------
// The operand loader of both kernels: the state of one 256 x 256 tile and the LDS-DMA that stages its K-tiles.
//
// A K-tile (64 channels of 256 A rows and 256 B rows) is staged as four 16-KB half-operands, {A, B} x {channels 0-31,
// 32-63}: 256 rows x 64 B each.  A wave-instruction of `buffer_load ... lds` writes 1 KiB = 16 rows x 64 B, and a wave
// stages two such pieces per half-operand: lane l fills LDS slot (row, l & 3) of rows piece * 16 + (l >> 2), piece =
// 2 * wave + q.  The 16-byte chunk a slot holds is XOR-swizzled on the SOURCE side, chunk = (l & 3) ^ f(row) with
// f(row) = (row >> 2) & 3 = (l >> 4) & 3, and the kernels' fragment reads apply the same involution.  What a lane needs
// per tile is therefore two byte offsets per operand (+ the frames t +- 1 of a shifted source, + the valid-tap mask of a
// 3x3), relative to windows that start at the tile's first frame / weight row: 32-bit offsets whatever the batch.
// ---------------------------------------------------------------------------------------------
template <int KS, bool SHIFT, bool DUAL, bool SHIFT2 = false> struct Tile256State {
  unsigned a_off[2], b_off[2];
  unsigned a_mask[KS == 3 ? 2 : 1];
  unsigned a_offp[SHIFT ? 2 : 1], a_offm[SHIFT ? 2 : 1];
  unsigned a_off2[DUAL ? 2 : 1];
  unsigned a_off2p[SHIFT2 ? 2 : 1], a_off2m[SHIFT2 ? 2 : 1];   // block placement: x2's frames t+1 / t-1
  int m0, n0;
  // (the operand windows as plain pointers + sizes: the host pass cannot hold __amdgpu_buffer_rsrc_t in a struct; the
  //  descriptors are rebuilt where they are used -- scalar moves)
  const char *pa, *pb, *pa2;
  int sza, sza2;
};

// What a kernel computes once and the loader reads per tile / per stage
struct Tile256Launch {
  int HoWo, frame_bytes, frame_bytes2;   // output pixels per frame; bytes per frame of x and (DUAL) of x2
  int nt1;                               // DUAL: K-tiles of the first source
  int wave, lane, chunk;                 // chunk: the global 16-B chunk held by this lane's LDS slot
};

// The loader state of output tile `tile` (row-major over ntm x ntn).  SHIFT: the A loader's temporal shift (conv1); DUAL:
// the K-concatenated second source x2 (conv3 + downsample as one GEMM, K = [conv3 input channels | block input channels]);
// SHIFT2: x2 read through the shift (block placement).
template <int KS, bool SHIFT, bool DUAL, bool SHIFT2>
__device__ __forceinline__ void tile256_setup(Tile256State<KS, SHIFT, DUAL, SHIFT2> &T, const ConvParams &p, const Tile256Launch &L, int tile) {
  const int tm = tile / p.ntn, tn = tile - tm * p.ntn;
  T.m0 = tm * 256;
  T.n0 = tn * 256;
  const int n_first = T.m0 / L.HoWo;
  const int frame0 = SHIFT ? (n_first > 0 ? n_first - 1 : 0) : n_first;
  const size_t a_bytes = ((size_t)p.N - frame0) * (size_t)L.frame_bytes;
  T.pa = reinterpret_cast<const char *>(p.x) + (size_t)frame0 * L.frame_bytes;
  T.sza = window_bytes(a_bytes);
  T.pb = reinterpret_cast<const char *>(p.w) + (size_t)T.n0 * p.Kp * 2;
  const int frame02 = (SHIFT2 && n_first > 0) ? n_first - 1 : n_first;
  const size_t a2_bytes = DUAL ? ((size_t)p.N - frame02) * (size_t)L.frame_bytes2 : 0;
  T.pa2 = reinterpret_cast<const char *>(DUAL ? p.x2 : p.x) + (size_t)frame02 * L.frame_bytes2;
  T.sza2 = window_bytes(a2_bytes);
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    const int row = (2 * L.wave + q) * 16 + (L.lane >> 2);
    const int m = T.m0 + row;
    const bool ok = m < p.M;
    const int mm = ok ? m : T.m0;
    const int n = mm / L.HoWo, rem = mm - n * L.HoWo;
    const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
    const int iy0 = oy * p.stride - p.pad, ix0 = ox * p.stride - p.pad;
    const int base = (n - frame0) * L.frame_bytes + (iy0 * p.Wi + ix0) * p.C * 2 + L.chunk * 16;
    T.a_off[q] = (KS == 1 && !ok) ? kInvalid : (unsigned)base;
    if (KS == 3) {
      unsigned mask = 0;
#pragma unroll
      for (int ky = 0; ky < 3; ++ky)
#pragma unroll
        for (int kx = 0; kx < 3; ++kx)
          if ((unsigned)(iy0 + ky) < (unsigned)p.Hi && (unsigned)(ix0 + kx) < (unsigned)p.Wi) mask |= 1u << (ky * 3 + kx);
      T.a_mask[q] = ok ? mask : 0u;
    }
    if (SHIFT) {
      const int t = n % p.T;
      T.a_offp[q] = (ok && t < p.T - 1) ? (unsigned)(base + L.frame_bytes) : kInvalid;
      T.a_offm[q] = (ok && t > 0) ? (unsigned)(base - L.frame_bytes) : kInvalid;
    }
    if (DUAL)
      T.a_off2[q] = ok ? (unsigned)((n - frame02) * L.frame_bytes2 + (oy * p.stride2 * p.Wi2 + ox * p.stride2) * p.C2 * 2 + L.chunk * 16)
                       : kInvalid;
    if (SHIFT2) {
      const int t = n % p.T;
      T.a_off2p[q] = (ok && t < p.T - 1) ? T.a_off2[q] + (unsigned)L.frame_bytes2 : kInvalid;
      T.a_off2m[q] = (ok && t > 0) ? T.a_off2[q] - (unsigned)L.frame_bytes2 : kInvalid;
    }
    T.b_off[q] = (unsigned)(row * p.Kp * 2 + L.chunk * 16);
  }
}

// Stage one half-operand of K-tile kt of the tile with state T into operand buffer `par` (0 / 1) of `lds`: which = 0 A k0-31,
// 1 B k0-31, 2 A k32-63, 3 B k32-63 (two 1-KiB pieces per wave); dead = kInvalid: zeros, no memory traffic
template <int KS, bool SHIFT, bool DUAL, bool SHIFT2>
__device__ __forceinline__ void tile256_stage(unsigned char *lds, const Tile256State<KS, SHIFT, DUAL, SHIFT2> &T, const ConvParams &p,
                                              const Tile256Launch &L, int kt, unsigned par, int which, unsigned dead) {
  typedef __attribute__((address_space(3))) void lds_void;
  const int kh = which >> 1;
  const unsigned kbytes = (unsigned)kt * 128u + (unsigned)kh * 64u;
  unsigned char *dst = lds + par * 65536u + ((which & 1) * 2 + kh) * 16384 + L.wave * 2048;
  const __amdgpu_buffer_rsrc_t rsrcA = buffer_fixed(T.pa, T.sza);
  const __amdgpu_buffer_rsrc_t rsrcB = buffer_fixed(T.pb, 256 * p.Kp * 2);
  const __amdgpu_buffer_rsrc_t rsrcA2 = buffer_fixed(T.pa2, T.sza2);
  if (which & 1) {
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcB, (lds_void *)(dst + q * 1024), 16, (int)(T.b_off[q] | dead), (int)kbytes, 0, 0);
  } else if (KS == 1) {
    unsigned mp = 0u, mm_ = 0u, m0_ = ~0u;
    if (SHIFT || SHIFT2) {
      const int c = kt * 64 + kh * 32 + L.chunk * 8 - (SHIFT2 ? L.nt1 * 64 : 0);   // first channel of this lane's chunk (of x2)
      mp = 0u - (unsigned)(c < p.fold);
      mm_ = (0u - (unsigned)(c < 2 * p.fold)) & ~mp;
      m0_ = ~(mp | mm_);
    }
    const bool second = DUAL && kt >= L.nt1;              // wave-uniform: which source this K-tile comes from
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      unsigned off = T.a_off[q];
      if (SHIFT) off = (T.a_offp[q] & mp) | (T.a_offm[q] & mm_) | (T.a_off[q] & m0_);
      unsigned off2 = T.a_off2[q];
      if (SHIFT2) off2 = (T.a_off2p[q] & mp) | (T.a_off2m[q] & mm_) | (T.a_off2[q] & m0_);
      if (DUAL && second)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcA2, (lds_void *)(dst + q * 1024), 16, (int)(off2 | dead),
                                                 (int)(kbytes - (unsigned)L.nt1 * 128u), 0, 0);
      else
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcA, (lds_void *)(dst + q * 1024), 16, (int)(off | dead), (int)kbytes, 0, 0);
    }
  } else {
    const int tap = (kt * 64) >> (p.logC4 + 2);           // C >= 64: a K-tile never straddles a tap
    const int ky = tap / 3, kx = tap - ky * 3;
    const unsigned tap_off = (unsigned)(((ky * p.Wi + kx) * p.C + (kt * 64 - tap * p.C) + kh * 32) * 2);
#pragma unroll
    for (int q = 0; q < 2; ++q)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrcA, (lds_void *)(dst + q * 1024), 16,
                                               (int)((((T.a_mask[q] >> tap) & 1u) ? T.a_off[q] + tap_off : kInvalid) | dead), 0, 0, 0);
  }
}

// ---------------------------------------------------------------------------------------------
// conv_bf16_256: the bf16 implicit GEMM on a 256 x 256 tile, ONE 8-wave workgroup per CU, operands staged by LDS-DMA.
//
// Why: the 128 x 128 bf16 tiles of conv_igemm are LDS-bound -- per MFMA they need as many LDS-array cycles
// (VGPR-staged ds_write_b128 of both operands + fragment reads) as the matrix pipe gives, and one barrier + full
// vmcnt drain per K-step on top (profiles/r01_bf16_pmc_sq_summary.txt: MFMA busy 0.27-0.34).  This kernel is the
// structure cdna_hip_programming.md prescribes for that regime:
//   * 256 x 256 output tile, K-tile 64 channels, 8 waves as 2 (M) x 4 (N), 128 x 64 per wave = 4 x 2 MFMA tiles of
//     v_mfma_f32_32x32x16_bf16: a quarter of the staging bytes and 3/4 of the fragment reads per MFMA of the 128^2 tile;
//   * both operands go global -> LDS by `buffer_load ... lds` (no VGPR round trip, no ds_write): a wave-instruction
//     writes 1 KiB = 16 rows x 64 B; the 16-byte chunk a lane fetches is XOR-swizzled on the SOURCE side with
//     f(row) = (row >> 2) & 3 and the fragment reads apply the same involution: ds_read_b128 is conflict-free;
//   * a K-tile is cut in four 16-KB "half-operands" by K, not by rows -- {A, B} x {channels 0-31, 32-63} -- because the
//     four phases of a K-tile each multiply ONE k16 group (6 ds_read_b128 + 8 MFMAs per wave): the k 0-31 halves are
//     dead after phase 1 and are re-filled (for K-tile t+2) in phases 2 and 3, the k 32-63 halves in phases 0 and 1 of
//     the next K-tile.  Two 64-KB buffers, FOUR half-operands always in flight, retired by a counted
//     `s_waitcnt vmcnt(8)` twice per K-tile -- never vmcnt(0) inside the loop -- and raw s_barriers;
//   * the two waves of a SIMD run STAGGERED by one barrier (waves 4-7 behind waves 0-3): one is in its 8-MFMA cluster
//     while the other reads fragments and issues DMA, instead of both queueing on the matrix pipe together;
//   * K-tiles past the end of K are staged with an out-of-range offset (zeros, no memory traffic), so the loop and
//     its wait counts are branch-free.
// Per output the products enter the accumulator in conv_igemm's order (k16 groups ascending), so results are
// bit-identical to the other bf16 tiles.  Epilogue: accumulators -> wave-private LDS slab (no workgroup barrier)
// -> + bias, ReLU, bf16, 16-byte stores of whole 128-byte row segments.
// Needs Cout % 256 == 0 and C % 64 == 0.  Template arms: KS = 3; KS = 1 with the fused temporal shift (conv1), with a
// residual (conv3) or with the K-concatenated second source (conv3 + downsample).  The tuner picks it where it wins
// (at least about one tile per CU; long K helps: conv2 and conv1 of layer3-4 at the config-5 size).
// ---------------------------------------------------------------------------------------------
template <int KS, bool SHIFT, bool RES = false, bool DUAL = false>
__global__ void __launch_bounds__(512, 1) conv_bf16_256_kernel(const ConvParams p) {
  static_assert(KS == 1 || KS == 3, "1x1 (optionally temporally shifted) and 3x3");
  static_assert(!(RES || DUAL) || (KS == 1 && !SHIFT), "residual / K-concatenated second source: plain 1x1 convs (conv3)");
  static_assert(!(RES && DUAL), "the fused conv3 + downsample GEMM has no residual");
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // 2 buffers x 64 KB; epilogue: 8 x 8704 B
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int half = lane >> 5, l31 = lane & 31;

  const int nwg = gridDim.x, bid = blockIdx.x;
  int tile = xcd_chunked32(bid, nwg);
  if (p.reverse) tile = nwg - 1 - tile;

  const Tile256Launch L = {p.Ho * p.Wo, p.Hi * p.Wi * p.C * 2, DUAL ? p.Hi2 * p.Wi2 * p.C2 * 2 : 0, DUAL ? p.K1 / 64 : 0,
                           wave, lane, (lane & 3) ^ ((lane >> 4) & 3)};
  Tile256State<KS, SHIFT, DUAL> T;
  tile256_setup(T, p, L, tile);
  const int m0 = T.m0, n0 = T.n0;
  const int nt = p.Kp / 64;                               // K-tiles
  // Stage one half-operand of K-tile kt (tile256_stage) into the buffer of its parity; K-tiles past the end: zeros
  auto stage = [&](int kt, int which) {
    const unsigned dead = (~(unsigned)((kt - nt) >> 31)) & kInvalid;
    tile256_stage(lds, T, p, L, kt, (unsigned)(kt & 1), which, dead);
  };

  f32x16 acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  // fragment addresses: row * 64 B + swizzled chunk; k16 group g reads chunk 2 * (g & 1) + half of region g >> 1
  const int sw = (l31 >> 2) & 3;
  const unsigned a_rd0 = (unsigned)((wm * 128 + l31) * 64 + ((0 + half) ^ sw) * 16);
  const unsigned a_rd1 = (unsigned)((wm * 128 + l31) * 64 + ((2 + half) ^ sw) * 16);
  const unsigned b_rd0 = (unsigned)(32768 + (wn * 64 + l31) * 64 + ((0 + half) ^ sw) * 16);
  const unsigned b_rd1 = (unsigned)(32768 + (wn * 64 + l31) * 64 + ((2 + half) ^ sw) * 16);

  // prologue: the six half-operands the schedule has in flight before K-tile 0 starts
  stage(0, 0); stage(0, 1); stage(0, 2); stage(0, 3); stage(1, 0); stage(1, 1);
  asm volatile("s_waitcnt vmcnt(8)" ::: "memory");        // K-tile 0, k 0-31 of A and B have landed (this wave's share)
  __builtin_amdgcn_s_barrier();
  // Stagger: waves 4-7 (wm == 1; the second wave of every SIMD) run one barrier behind waves 0-3, so that on each
  // SIMD one wave is in its MFMA cluster while its partner reads fragments / issues DMA -- in lockstep both would
  // read together and then queue on the one matrix pipe (MI355X_MICROARCH.md, two waves per SIMD, item 9).
  // Consequences for the hand-placed synchronisation: (a) the counted vmcnt sits BEFORE the first barrier of the odd
  // phases, so that the delayed group too has retired its DMA one barrier before the early group reads the data;
  // (b) the fragment reads are retired (lgkmcnt(0)) before the first barrier of their phase, so that the DMA which the
  // early group issues one phase later cannot overtake a read of the delayed group.
  if (wm == 1) __builtin_amdgcn_s_barrier();

  for (int kt = 0; kt < nt; ++kt) {
    const unsigned buf = (unsigned)(kt & 1) * 65536u;
#pragma unroll
    for (int ph = 0; ph < 4; ++ph) {
      u32x4 af[4], bf[2];
      {
        const unsigned ra = buf + (ph >> 1) * 16384u + ((ph & 1) ? a_rd1 : a_rd0);
        const unsigned rb = buf + (ph >> 1) * 16384u + ((ph & 1) ? b_rd1 : b_rd0);
#pragma unroll
        for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const u32x4 *>(lds + rb + j * 2048);
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const u32x4 *>(lds + ra + i * 2048);
      }
      // refill what the previous phases have finished reading: k 32-63 halves of the OTHER buffer (K-tile kt+1) in
      // phases 0-1, k 0-31 halves of THIS buffer (K-tile kt+2) in phases 2-3
      if (ph == 0) stage(kt + 1, 2);
      else if (ph == 1) stage(kt + 1, 3);
      else if (ph == 2) stage(kt + 2, 0);
      else stage(kt + 2, 1);
      // odd phases: the counted wait that retires the two half-operands the NEXT phase reads (8 = the four younger
      // half-operands x 2 pieces per wave stay in flight; never 0 inside the loop)
      if (ph & 1) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");
      else asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_s_setprio(1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i]), __builtin_bit_cast(bf16x8, bf[j]),
                                                              acc[i][j], 0, 0, 0);
      __builtin_amdgcn_s_setprio(0);
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
    }
  }
  if (wm == 0) __builtin_amdgcn_s_barrier();              // the early group waits for the delayed one
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the dead tail stages (zeros) must land before LDS is reused
  __builtin_amdgcn_s_barrier();

  // ---- epilogue: per wave, four 32 x 64 slabs through a private LDS region ---------------------------------
  float *Cs = reinterpret_cast<float *>(lds + wave * 8704);  // [32][68] fp32
  const size_t y_bytes = ((size_t)p.M - m0) * p.Cout * 2;
  const __amdgpu_buffer_rsrc_t rsrcY = buffer_window(reinterpret_cast<char *>(p.y) + (size_t)m0 * p.Cout * 2, y_bytes);
  const float floor_ = p.relu ? 0.f : -INFINITY;
  const int c8 = lane & 7, r8l = lane >> 3;
  const f32x4 bias0 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + wn * 64 + c8 * 8);
  const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(p.bias + n0 + wn * 64 + c8 * 8 + 4);
  // residual (RES): the 8 channels of this lane's row segment, fetched one slab ahead of their use
  const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(reinterpret_cast<const char *>(RES ? p.res : p.y) + (size_t)m0 * p.Cout * 2, y_bytes);
  u32x4 rres[2][RES ? 4 : 1];
  auto load_res = [&](int i, int set) {
    if constexpr (RES) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        rres[set][k] = __builtin_amdgcn_raw_buffer_load_b128(
            rsrcR, ((wm * 128 + i * 32 + r8l + 8 * k) * p.Cout + n0 + wn * 64 + c8 * 8) * 2, 0, 0);
    }
  };
  load_res(0, 0);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (i + 1 < 4) load_res(i + 1, (i + 1) & 1);
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) Cs[((e & 3) + 8 * (e >> 2) + 4 * half) * 68 + j * 32 + l31] = acc[i][j][e];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (same wave wrote it: no barrier needed)
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int rr = r8l + 8 * k;
      const f32x4 c0 = *reinterpret_cast<const f32x4 *>(Cs + rr * 68 + c8 * 8);
      const f32x4 c1 = *reinterpret_cast<const f32x4 *>(Cs + rr * 68 + c8 * 8 + 4);
      float v[8] = {c0[0] + bias0[0], c0[1] + bias0[1], c0[2] + bias0[2], c0[3] + bias0[3],
                    c1[0] + bias1[0], c1[1] + bias1[1], c1[2] + bias1[2], c1[3] + bias1[3]};
      if constexpr (RES) {
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += split_elem(rres[i & 1][k], e);
      }
      u32x4 o;
#pragma unroll
      for (int w2 = 0; w2 < 4; ++w2) o[w2] = pack_bf16(fmaxf(v[2 * w2], floor_), fmaxf(v[2 * w2 + 1], floor_));
      const int row = wm * 128 + i * 32 + rr;
      __builtin_amdgcn_raw_buffer_store_b128(o, rsrcY, (row * p.Cout + n0 + wn * 64 + c8 * 8) * 2, 0, TSM_AUX_256);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // slab reads done before the next slab overwrites it
  }
}

// ---------------------------------------------------------------------------------------------
// conv_bf16_256p: conv_bf16_256's K pipeline run PERSISTENTLY over the tiles of a workgroup, without ever draining.
//
// Why: conv_bf16_256 is one 128-KB workgroup per CU, so nothing overlaps a tile's prologue (the first operands' HBM
// latency, 2-3 us) or its epilogue (accumulators through LDS, residual loads, stores) -- and with short K that is a
// third of a tile (K = 256: four K-tiles = 3.4 us of MFMA per 17-us tile; the 1x1 launches of layer3/4 sit at 3.0-4.3
// TB/s and 0.29-0.44 of the MFMA peak: neither roofline).  Here
//   * the K-tile sequence is FLAT across tiles: the refills the last two K-tiles of tile s issue ("K-tile kt + 1,
//     kt + 2") are the first K-tiles of tile s + 1, staged from that tile's loader state (two sets of lane offsets and
//     descriptors, current / next); the four-half-operands-in-flight schedule, its counted waits, the staggered wave
//     groups and the barriers are conv_bf16_256's, unchanged, and run from the first K-tile of the first tile to the
//     last K-tile of the last;
//   * the epilogue leaves the two operand buffers alone, so it can sit between two K-tiles while the next tile's operands
//     land.  Without a residual it touches no LDS at all: the product is TRANSPOSED (A = weights, B = pixels: the fragment
//     formats are symmetric, the products of an output enter its accumulator in the same k order -> same bits), a lane
//     then holds 4-channel runs of ONE pixel, and bias + ReLU + bf16 + v_permlane32_swap give 16-byte stores straight
//     from registers (conv3x3_ws's epilogue; measured against the slab form below: 3-6 % faster on these arms).  With a
//     residual the product is not transposed and the epilogue goes through eight wave-private [8][68] fp32 SUB-SLABS
//     behind the bias (whole 128-byte row segments of residual and output per 8 lanes; the register form, 16 bytes per
//     lane and two lanes per pixel, lost to conv_bf16_256 on exactly these launches), residual eight sub-slabs ahead;
//     the bias of all Cout channels sits in LDS behind the two buffers;
//   * the 16 stores of an epilogue are younger than the operands the next K-tile waits for: its two counted waits
//     are vmcnt(8 + 16) instead of vmcnt(8) (vector-memory operations retire in order; a vmcnt(8) there would wait
//     for the stores' completion); the residual arm requests sub-slabs 0-7 at the START of the tile's last K-tile,
//     whose waits are therefore vmcnt(8 + 8).
// Needs at least two K-tiles per tile (K >= 128: "kt + 2" must not skip a tile) and Cout <= 2048 (the bias in LDS).
// Bit-identical to conv_bf16_256 and to conv_igemm's bf16 tiles; the tuner picks per layer.
// ---------------------------------------------------------------------------------------------
#ifndef TSM_256P_STAMP
#define TSM_256P_STAMP 0   // diagnostic builds only: per-phase cycle sums of workgroup 0 (s_memtime), printed at the kernel's end (1: conv3 + downsample, 2: 3x3)
#endif
constexpr size_t kLds256pBytes = 131072 + 8192 + 8 * 2176;   // two operand buffers | bias [<= 2048] fp32 | residual arm: eight [8][68] fp32 sub-slabs

template <int KS, bool SHIFT, bool RES = false, bool DUAL = false>
__global__ void __launch_bounds__(512, 1) conv_bf16_256p_kernel(const ConvParams p) {
  static_assert(KS == 1 || KS == 3, "1x1 (optionally temporally shifted) and 3x3");
  static_assert(!(RES || DUAL) || KS == 1, "residual / K-concatenated second source: plain 1x1 convs (conv3)");
  static_assert(!(RES && DUAL), "the fused conv3 + downsample GEMM has no residual");
  // SHIFT with RES / DUAL is block placement (tsm_igemm.hip, BSHIFT): the identity -- the residual, or the second source --
  // is read through the temporal shift and the first source is not
  constexpr bool ASHIFT = SHIFT && !RES && !DUAL;   // the A loader's shift (conv1)
  constexpr bool RSHIFT = SHIFT && RES, XSHIFT = SHIFT && DUAL;
  TSM_STAMP_DECL(TSM_256P_STAMP, 6);
  extern __shared__ __attribute__((aligned(16))) unsigned char lds[];   // 2 buffers x 64 KB | bias [Cout] fp32
  typedef Tile256State<KS, ASHIFT, DUAL, XSHIFT> State;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave >> 2, wn = wave & 3;
  const int half = lane >> 5, l31 = lane & 31;

  const int ntiles = p.ntm * p.ntn, nwg = (int)gridDim.x, bid = (int)blockIdx.x;
  const int my = (ntiles - bid + nwg - 1) / nwg;          // tiles of this workgroup (>= 1: the grid never exceeds the tiles)
  const int HoWo = p.Ho * p.Wo;
  const Tile256Launch L = {HoWo, p.Hi * p.Wi * p.C * 2, DUAL ? p.Hi2 * p.Wi2 * p.C2 * 2 : 0, DUAL ? p.K1 / 64 : 0,
                           wave, lane, (lane & 3) ^ ((lane >> 4) & 3)};
  const int nt = p.Kp / 64;                               // K-tiles per tile (>= 2)

  float *bias_lds = reinterpret_cast<float *>(lds + 131072);
  for (int i = tid; i < p.Cout; i += 512) bias_lds[i] = p.bias[i];

  // the s-th tile of this workgroup (virtual block bid + s * nwg in conv_bf16_256's XCD-chunked order)
  auto tile_of = [&](int s) {
    int tile = xcd_chunked32(bid + s * nwg, ntiles);
    if (tile >= ntiles) tile = ntiles - 1;                // (s == my: never staged live, kept in range for the arithmetic)
    return p.reverse ? ntiles - 1 - tile : tile;
  };

  f32x16 acc[4][2];      // acc[i][j]: rows = channels n0 + 64 wn + 32 j + .., columns = pixels m0 + 128 wm + 32 i + l31
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

  const int sw = (l31 >> 2) & 3;
  const unsigned a_rd0 = (unsigned)((wm * 128 + l31) * 64 + ((0 + half) ^ sw) * 16);
  const unsigned a_rd1 = (unsigned)((wm * 128 + l31) * 64 + ((2 + half) ^ sw) * 16);
  const unsigned b_rd0 = (unsigned)(32768 + (wn * 64 + l31) * 64 + ((0 + half) ^ sw) * 16);
  const unsigned b_rd1 = (unsigned)(32768 + (wn * 64 + l31) * 64 + ((2 + half) ^ sw) * 16);
  const float floor_ = p.relu ? 0.f : -INFINITY;

  // Residual arm (RES): the product is NOT transposed and the epilogue goes through LDS like conv_bf16_256's -- whole
  // 128-byte row segments of the residual and of the output per 8 lanes; the transposed register epilogue would fetch the
  // residual as 16 bytes per lane, two lanes per pixel, and lost to conv_bf16_256 on exactly these launches -- but in
  // SUB-SLABS of 8 rows x 64 channels ([8][68] fp32 per wave = 17 KB for the workgroup, behind the bias): the two operand
  // buffers stay untouched, so the next tile's operands still land under the epilogue.  A wave tile is 16 sub-slabs; the
  // residual of sub-slab t is ONE 16-byte load per lane (row t * 8 + lane / 8, channels 8 (lane % 8) ..), eight of
  // them in flight: sub-slabs 0-7 are requested at the START of the tile's last K-tile -- older than that K-tile's four
  // operand stages, so that consuming them does not wait for the next tile's operands (vector-memory operations retire
  // in order) -- and sub-slab t + 8 when sub-slab t has been consumed.
  u32x4 rres[RES ? 8 : 1];
  const int c8 = lane & 7, r8l = lane >> 3;
  auto load_res = [&](const State &T, int t, int slot) {
    if constexpr (RSHIFT) {
      // block placement: row r of the identity reads row r + Ho*Wo (channels [0, fold); zeros at the clip's last frame),
      // r - Ho*Wo ([fold, 2 fold); zeros at its first frame) or r -- one frame either side of the tile's window
      const int rbase = T.m0 >= HoWo ? T.m0 - HoWo : 0;
      const size_t y_bytes = ((size_t)p.M - rbase) * p.Cout * 2;
      const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(reinterpret_cast<const char *>(p.res) + (size_t)rbase * p.Cout * 2, y_bytes);
      const int row = wm * 128 + t * 8 + r8l, c = T.n0 + wn * 64 + c8 * 8;
      const int tt = ((T.m0 + row) / HoWo) % p.T;
      unsigned o = (unsigned)(((T.m0 - rbase + row) * p.Cout + c) * 2);
      const unsigned step = (unsigned)(HoWo * p.Cout * 2);
      if (c < p.fold) o = tt < p.T - 1 ? o + step : kInvalid;
      else if (c < 2 * p.fold) o = tt > 0 ? o - step : kInvalid;
      rres[slot] = __builtin_amdgcn_raw_buffer_load_b128(rsrcR, (int)o, 0, 0);
    } else if constexpr (RES) {
      const size_t y_bytes = ((size_t)p.M - T.m0) * p.Cout * 2;
      const __amdgpu_buffer_rsrc_t rsrcR = buffer_window(reinterpret_cast<const char *>(p.res) + (size_t)T.m0 * p.Cout * 2, y_bytes);
      rres[slot] = __builtin_amdgcn_raw_buffer_load_b128(
          rsrcR, ((wm * 128 + t * 8 + r8l) * p.Cout + T.n0 + wn * 64 + c8 * 8) * 2, 0, 0);
    }
  };

  State cur, nxt;
  tile256_setup(cur, p, L, tile_of(0));
  // prologue: the six half-operands the schedule has in flight before the first K-tile starts (nt >= 2: all of tile 0)
  tile256_stage(lds, cur, p, L, 0, 0u, 0, 0u); tile256_stage(lds, cur, p, L, 0, 0u, 1, 0u);
  tile256_stage(lds, cur, p, L, 0, 0u, 2, 0u); tile256_stage(lds, cur, p, L, 0, 0u, 3, 0u);
  tile256_stage(lds, cur, p, L, 1, 1u, 0, 0u); tile256_stage(lds, cur, p, L, 1, 1u, 1, 0u);
  asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");   // K-tile 0, k 0-31 of A and B have landed (this wave's share); the bias is written
  __builtin_amdgcn_s_barrier();
  if (wm == 1) __builtin_amdgcn_s_barrier();              // the stagger of conv_bf16_256: waves 4-7 one barrier behind

  int g = 0;                                              // K-tiles done so far: the LDS buffer of a K-tile is its parity
  for (int s = 0; s < my; ++s) {
    const unsigned next_dead = s + 1 < my ? 0u : kInvalid;
    TSM_STAMP(TSM_256P_STAMP, 5);
    tile256_setup(nxt, p, L, tile_of(s + 1));
    TSM_STAMP(TSM_256P_STAMP, 0);
    for (int kt = 0; kt < nt; ++kt, ++g) {
      const unsigned buf = (unsigned)(g & 1) * 65536u;
      // K-tile kt + d of the flat sequence: this tile's, or the first ones of the next tile
      auto stage = [&](int d, int which) {
        const unsigned par = (unsigned)((g + d) & 1);
        if (kt + d < nt) tile256_stage(lds, cur, p, L, kt + d, par, which, 0u);
        else tile256_stage(lds, nxt, p, L, kt + d - nt, par, which, next_dead);
      };
      auto stage_ph = [&](int ph) {
        if (ph == 0) stage(1, 2);
        else if (ph == 1) stage(1, 3);
        else if (ph == 2) stage(2, 0);
        else stage(2, 1);
      };
      const bool after_epilogue = kt == 0 && s > 0;       // 16 stores sit between the operands awaited here and the younger DMA
      const bool with_res = RES && kt == nt - 1;          // 8 residual loads sit there (issued right here)
      if (with_res) {
#pragma unroll
        for (int t = 0; t < 8; ++t) load_res(cur, t, t);
      }
      if constexpr (KS == 3) {
        // 3x3 arm (the 1x1 arms lose 0-3 % with it and keep one cluster per pair): one barrier pair per K-HALF: the twelve fragment reads and the four DMA pieces of both of its k-16 steps in front of the
        // first barrier, sixteen MFMAs (the same order as below: k 0-15 then k 16-31 of every accumulator) behind it.  The waits are
        // those of the odd phases below, behind the same operations.
#pragma unroll
        for (int pp = 0; pp < 2; ++pp) {
          u32x4 af[2][4], bf[2][2];
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2) {
            const unsigned ra = buf + pp * 16384u + (h2 ? a_rd1 : a_rd0);
            const unsigned rb = buf + pp * 16384u + (h2 ? b_rd1 : b_rd0);
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[h2][j] = *reinterpret_cast<const u32x4 *>(lds + rb + j * 2048);
#pragma unroll
            for (int i = 0; i < 4; ++i) af[h2][i] = *reinterpret_cast<const u32x4 *>(lds + ra + i * 2048);
          }
          stage_ph(2 * pp);
          stage_ph(2 * pp + 1);
          if (after_epilogue) wait_vmcnt_lgkm0<24>();
          else wait_vmcnt_lgkm0<8>();
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_barrier();
          __builtin_amdgcn_s_setprio(1);
#pragma unroll
          for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
              for (int j = 0; j < 2; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf[h2][j]), __builtin_bit_cast(bf16x8, af[h2][i]),
                                                                    acc[i][j], 0, 0, 0);
          __builtin_amdgcn_s_setprio(0);
          __builtin_amdgcn_sched_barrier(0);
          __builtin_amdgcn_s_barrier();
        }
      } else {
#pragma unroll
      for (int ph = 0; ph < 4; ++ph) {
        u32x4 af[4], bf[2];
        {
          const unsigned ra = buf + (ph >> 1) * 16384u + ((ph & 1) ? a_rd1 : a_rd0);
          const unsigned rb = buf + (ph >> 1) * 16384u + ((ph & 1) ? b_rd1 : b_rd0);
#pragma unroll
          for (int j = 0; j < 2; ++j) bf[j] = *reinterpret_cast<const u32x4 *>(lds + rb + j * 2048);
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = *reinterpret_cast<const u32x4 *>(lds + ra + i * 2048);
        }
        // the phase's two DMA pieces: in front of the barrier (the other wave group's MFMAs run meanwhile)
        stage_ph(ph);
        if (ph & 1) {
          if (after_epilogue) wait_vmcnt_lgkm0<24>();
          else if (with_res) wait_vmcnt_lgkm0<16>();
          else wait_vmcnt_lgkm0<8>();
        } else {
          asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        }
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 2; ++j)
            acc[i][j] = RES ? __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, af[i]), __builtin_bit_cast(bf16x8, bf[j]),
                                                                      acc[i][j], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, bf[j]), __builtin_bit_cast(bf16x8, af[i]),
                                                                      acc[i][j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
        __builtin_amdgcn_sched_barrier(0);
        __builtin_amdgcn_s_barrier();
      }
      }
      TSM_STAMP(TSM_256P_STAMP, (kt == 0 ? 1 : kt == 1 ? 2 : 3));
    }
    // ---- epilogue of tile s: the next tile's first operands are in flight ----
    if constexpr (!RES) {   // from registers (no LDS, no barrier)
      const size_t y_bytes = ((size_t)p.M - cur.m0) * p.Cout * 2;
      const int ysz = window_bytes(y_bytes);
      const __amdgpu_buffer_rsrc_t rsrcY = buffer_fixed(reinterpret_cast<char *>(p.y) + (size_t)cur.m0 * p.Cout * 2, ysz);
      const int cbase = (cur.n0 + wn * 64) * 2 + half * 32;               // this lane's first byte within a pixel's row
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int o = (wm * 128 + i * 32 + l31) * p.Cout * 2 + cbase;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          unsigned pk[4][2];
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const f32x4 b = *reinterpret_cast<const f32x4 *>(bias_lds + cur.n0 + wn * 64 + j * 32 + 8 * q + 4 * half);
#pragma unroll
            for (int w2 = 0; w2 < 2; ++w2) {
              float v0 = acc[i][j][4 * q + 2 * w2] + b[2 * w2], v1 = acc[i][j][4 * q + 2 * w2 + 1] + b[2 * w2 + 1];
              pk[q][w2] = pack_bf16(fmaxf(v0, floor_), fmaxf(v1, floor_));
            }
          }
#pragma unroll
          for (int qq = 0; qq < 2; ++qq)
#pragma unroll
            for (int w2 = 0; w2 < 2; ++w2) {
              const auto r2 = __builtin_amdgcn_permlane32_swap(pk[qq][w2], pk[qq + 2][w2], false, false);
              pk[qq][w2] = r2[0];
              pk[qq + 2][w2] = r2[1];
            }
#pragma unroll
          for (int qq = 0; qq < 2; ++qq) {
            const u32x4 ov = {pk[qq][0], pk[qq][1], pk[qq + 2][0], pk[qq + 2][1]};
            __builtin_amdgcn_raw_buffer_store_b128(ov, rsrcY, o, j * 64 + qq * 16, TSM_AUX_256);
          }
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
        }
      }
    } else {                // residual arm: 16 sub-slabs of 8 rows through this wave's [8][68] fp32 slab
      float *Cs = reinterpret_cast<float *>(lds + 131072 + 8192 + wave * 2176);
      const size_t y_bytes = ((size_t)p.M - cur.m0) * p.Cout * 2;
      const __amdgpu_buffer_rsrc_t rsrcY = buffer_window(reinterpret_cast<char *>(p.y) + (size_t)cur.m0 * p.Cout * 2, y_bytes);
      const f32x4 bias0 = *reinterpret_cast<const f32x4 *>(bias_lds + cur.n0 + wn * 64 + c8 * 8);
      const f32x4 bias1 = *reinterpret_cast<const f32x4 *>(bias_lds + cur.n0 + wn * 64 + c8 * 8 + 4);
#pragma unroll
      for (int t = 0; t < 16; ++t) {
        const int i = t >> 2, q = t & 3;          // rows 32 i + 8 q .. + 8 of the wave tile: accumulator elements 4 q .. 4 q + 3
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) Cs[(4 * half + r) * 68 + j * 32 + l31] = acc[i][j][4 * q + r];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // (same wave wrote it: no barrier needed)
        const f32x4 c0 = *reinterpret_cast<const f32x4 *>(Cs + r8l * 68 + c8 * 8);
        const f32x4 c1 = *reinterpret_cast<const f32x4 *>(Cs + r8l * 68 + c8 * 8 + 4);
        float v[8] = {c0[0] + bias0[0], c0[1] + bias0[1], c0[2] + bias0[2], c0[3] + bias0[3],
                      c1[0] + bias1[0], c1[1] + bias1[1], c1[2] + bias1[2], c1[3] + bias1[3]};
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] += split_elem(rres[t & 7], e);
        u32x4 o;
#pragma unroll
        for (int w2 = 0; w2 < 4; ++w2) o[w2] = pack_bf16(fmaxf(v[2 * w2], floor_), fmaxf(v[2 * w2 + 1], floor_));
        __builtin_amdgcn_raw_buffer_store_b128(o, rsrcY, ((wm * 128 + t * 8 + r8l) * p.Cout + cur.n0 + wn * 64 + c8 * 8) * 2, 0, TSM_AUX_256);
        if (t + 8 < 16) load_res(cur, t + 8, t & 7);
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");     // slab reads done before the next sub-slab overwrites it
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
          for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    }
    TSM_STAMP(TSM_256P_STAMP, 4);
    cur = nxt;
  }
#if TSM_256P_STAMP
  if (((TSM_256P_STAMP == 1 && DUAL) || (TSM_256P_STAMP == 2 && KS == 3)) && bid == 0 && (tid == 0 || tid == 256))
    printf("256p KS=%d DUAL=%d wave %d tiles=%d nt=%d: setup %llu ktile0 %llu ktile1 %llu ktiles2+ %llu epilogue %llu other %llu cycles\n", KS, (int)DUAL,
           wave, my, nt, stamp_acc[0], stamp_acc[1], stamp_acc[2], stamp_acc[3], stamp_acc[4], stamp_acc[5]);
#endif
  if (wm == 0) __builtin_amdgcn_s_barrier();              // the early group waits for the delayed one
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");        // the dead tail stages (zeros) land before the workgroup leaves its LDS
}

constexpr size_t kLds256Bytes = 131072;

// Both kernels.  The route (conv_bf16_256[p]_valid, tile counts, grid: tsm_conv_rules.h) names the family and the arm <KS, SHIFT, RES, DUAL>.
hipError_t launch_conv_bf16_256(const ConvParams &p, const ConvRoute &r, hipStream_t s) {
  const dim3 grid(r.grid), block(512);
  if (r.family == kFamBf16_256) {
    if (r.ks == 3) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256_kernel<3, false>), grid, block, kLds256Bytes, s, p);
    else if (r.shift) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256_kernel<1, true>), grid, block, kLds256Bytes, s, p);
    else if (r.res) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256_kernel<1, false, true, false>), grid, block, kLds256Bytes, s, p);
    else if (r.dual) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256_kernel<1, false, false, true>), grid, block, kLds256Bytes, s, p);
    else TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256_kernel<1, false>), grid, block, kLds256Bytes, s, p);
  } else if (r.ks == 3) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<3, false>), grid, block, kLds256pBytes, s, p);
  else if (r.shift && r.res) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, true, true, false>), grid, block, kLds256pBytes, s, p);
  else if (r.shift && r.dual) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, true, false, true>), grid, block, kLds256pBytes, s, p);
  else if (r.shift) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, true>), grid, block, kLds256pBytes, s, p);
  else if (r.res) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, false, true, false>), grid, block, kLds256pBytes, s, p);
  else if (r.dual) TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, false, false, true>), grid, block, kLds256pBytes, s, p);
  else TSM_KLAUNCH_WALK(p.reverse, (conv_bf16_256p_kernel<1, false>), grid, block, kLds256pBytes, s, p);
  return hipGetLastError();
}

hipError_t opt_in_bf16_256() {
  OptIn opt_in;
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256_kernel<1, false>), kLds256Bytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256_kernel<1, true>), kLds256Bytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256_kernel<3, false>), kLds256Bytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256_kernel<1, false, true, false>), kLds256Bytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256_kernel<1, false, false, true>), kLds256Bytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, false>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, true>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<3, false>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, false, true, false>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, false, false, true>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, true, true, false>), kLds256pBytes);
  opt_in(reinterpret_cast<const void *>(&conv_bf16_256p_kernel<1, true, false, true>), kLds256pBytes);
  return opt_in.first;
}

}  // namespace tsm
