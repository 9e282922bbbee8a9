// The position-major form of the segmented fp32 3x3 launch (ConvParams::pos_major) on the CPU, under ASAN + UBSAN: the pure
// functions of csrc/tsm_conv_rules.h that conv_igemm<.., kPrecF32 | kPrecPosMajor, ..> and splitk_reduce_pos_kernel inline --
// pos_major_row, pos_major_tap_mask, next_live_kstep -- and pos_major_valid / conv_route, which decide where the arm runs.
// A stand-alone program (tests/test_pos_major_cpu.py builds and runs it):
//   1. the row map m' -> frame * HoWo + position is a bijection of [0, M), and a 64-row tile holds one position;
//   2. pos_major_valid refuses each excluded form, and conv_route then runs the natural order with the same tiles and grid;
//   3. the live walk visits exactly the K-steps whose tap is in bounds, in increasing order, from any segment start, and the
//      kernel's loop (restated below) cuts them into the natural arm's segments, skipping the segments without a live step;
//   4. the live shares of the headline's layers at N = 256 frames.
#include <cinttypes>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

static int g_fail = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_fail <= 20) {                      \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                     \
        printf("\n");                            \
      }                                          \
    }                                            \
  } while (0)

using tsm::ConvParams;

static float g_dummy = 0.f;

// A segmented fp32 3x3 layer as the engine launches it: n frames of hi x wi pixels, c -> cout channels.
static ConvParams layer(int n, int hi, int wi, int c, int cout, int stride) {
  const tsm_host::LayerGeom g = tsm_host::layer_geometry(c, 3, stride, tsm::kPrecF32);
  ConvParams p = tsm_host::conv_shape_params(g, 3, stride, cout, n, hi, wi, true, 0, 1, tsm::kPrecF32, false);
  p.tile = tsm::kTile64x64;
  p.pos_major = 1;
  return p;
}

// The K-steps whose tap reads inside the frame for output (oy, ox), from the definition of the convolution.
static std::vector<int> live_steps(const ConvParams &p, int oy, int ox) {
  std::vector<int> out;
  const int spt = p.C / 32;
  for (int kt = 0; kt < p.Kp / 32; ++kt) {
    const int tap = kt / spt, ky = tap / 3, kx = tap % 3;
    const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
    if (iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi) out.push_back(kt);
  }
  return out;
}

// conv_igemm's position-major K loop, restated: the steps it multiplies, one vector per flushed segment; `loads` = every step
// a load was issued for (the prologue's two and the injected ones; nk = a dead step).
static std::vector<std::vector<int>> kernel_walk(unsigned mask, int spt, int kt0, int nk, int seg_len, std::vector<int> *loads) {
  std::vector<std::vector<int>> segs;
  int kt = tsm::next_live_kstep(kt0, mask, spt, nk);
  int kt1 = tsm::next_live_kstep(kt + 1, mask, spt, nk);
  loads->push_back(kt);
  loads->push_back(kt1);
  while (kt < nk) {
    const int bound = (kt / seg_len + 1) * seg_len, kend = bound < nk ? bound : nk;
    std::vector<int> seg;
    while (kt < kend) {
      const int kt2 = tsm::next_live_kstep(kt1 + 1, mask, spt, nk);
      loads->push_back(kt2);
      seg.push_back(kt);
      kt = kt1;
      kt1 = kt2;
    }
    segs.push_back(seg);
  }
  return segs;
}

static void check_shape(int hi, int wi, int stride, int c) {
  for (int n : {64, 128}) {
    const ConvParams p = layer(n, hi, wi, c, 64, stride);
    EXPECT(tsm::pos_major_valid(p, 3), "%dx%d s%d c%d n%d must be valid", hi, wi, stride, c, n);
    const int howo = p.Ho * p.Wo;
    // 1. the row map
    std::vector<char> seen((size_t)p.M, 0);
    for (int m = 0; m < p.M; ++m) {
      int frame = -1, pos = -1, f0 = -1, p0 = -1;
      tsm::pos_major_row(m, p.N, &frame, &pos);
      tsm::pos_major_row(m / 64 * 64, p.N, &f0, &p0);
      EXPECT(frame >= 0 && frame < p.N && pos >= 0 && pos < howo, "row %d -> frame %d position %d", m, frame, pos);
      EXPECT(pos == p0 && frame == f0 + m % 64, "row %d: its tile starts at frame %d position %d, it is frame %d position %d", m, f0, p0, frame, pos);
      const int64_t y = (int64_t)frame * howo + pos;
      if (y < 0 || y >= p.M) { EXPECT(false, "row %d -> y row %" PRId64 " outside [0, %d)", m, y, p.M); continue; }
      EXPECT(!seen[(size_t)y], "y row %" PRId64 " written twice", y);
      seen[(size_t)y] = 1;
    }
    for (int y = 0; y < p.M; ++y) EXPECT(seen[(size_t)y], "y row %d never written", y);
    if (n != 64) continue;
    // 3. the live walk of every position
    const int nk = p.Kp / 32, spt = p.C / 32, seg_len = p.kseg_len;
    EXPECT(seg_len > 0 && nk == 9 * spt, "c %d: %d K-steps, segments of %d", c, nk, seg_len);
    for (int pos = 0; pos < howo; ++pos) {
      const unsigned mask = tsm::pos_major_tap_mask(pos, p.Wo, p.Hi, p.Wi, p.stride, p.pad);
      const std::vector<int> want = live_steps(p, pos / p.Wo, pos % p.Wo);
      EXPECT((mask & ~0x1ffu) == 0 && (mask & 0x10u), "position %d: mask %#x (the centre tap is always live)", pos, mask);
      EXPECT((int)want.size() == __builtin_popcount(mask) * spt, "position %d: %zu live steps, mask %#x", pos, want.size(), mask);
      // from any segment start, to the end of K (a whole tile: start 0) and to the end of that segment (a tail piece)
      for (int kt0 = 0; kt0 < nk; kt0 += seg_len)
        for (int end : {nk, kt0 + seg_len < nk ? kt0 + seg_len : nk}) {
          std::vector<int> exp;
          for (int k : want)
            if (k >= kt0 && k < end) exp.push_back(k);
          std::vector<int> got;
          for (int kt = tsm::next_live_kstep(kt0, mask, spt, end); kt < end; kt = tsm::next_live_kstep(kt + 1, mask, spt, end)) {
            if (got.size() > (size_t)nk) break;
            got.push_back(kt);
          }
          EXPECT(got == exp, "%dx%d s%d c%d position %d from step %d to %d: %zu steps walked, %zu live", hi, wi, stride, c, pos, kt0, end, got.size(), exp.size());
          std::vector<int> loads;
          const std::vector<std::vector<int>> segs = kernel_walk(mask, spt, kt0, end, seg_len, &loads);
          std::vector<int> flat;
          int last_seg = -1;
          for (const std::vector<int> &s : segs) {
            EXPECT(!s.empty(), "position %d from %d: an empty segment was flushed", pos, kt0);
            for (int k : s) {
              EXPECT(s.empty() || k / seg_len == s[0] / seg_len, "position %d: steps %d and %d in one segment", pos, s[0], k);
              flat.push_back(k);
            }
            if (!s.empty()) { EXPECT(s[0] / seg_len > last_seg, "position %d: segments out of order", pos); last_seg = s[0] / seg_len; }
          }
          EXPECT(flat == exp, "%dx%d s%d c%d position %d from %d to %d: the kernel's loop multiplies %zu steps, %zu live", hi, wi, stride, c, pos, kt0, end, flat.size(), exp.size());
          // every load is of a live step or dead (== end), and the live ones are the walked steps in order, each once
          std::vector<int> live_loads;
          for (int k : loads) {
            EXPECT(k <= end, "a load of step %d past %d", k, end);
            if (k < end) live_loads.push_back(k);
          }
          EXPECT(live_loads == exp, "position %d from %d to %d: %zu live loads for %zu steps", pos, kt0, end, live_loads.size(), exp.size());
        }
    }
  }
}

static void check_refusals() {
  const ConvParams base = layer(128, 14, 14, 256, 256, 1);
  EXPECT(tsm::pos_major_valid(base, 3), "the base layer is valid");
  struct Row { const char *what; int ks; void (*edit)(ConvParams &); };
  const Row rows[] = {
      {"split-bf16", 3, [](ConvParams &p) { p.prec = tsm::kPrecBf16x3; }},
      {"bf16", 3, [](ConvParams &p) { p.prec = tsm::kPrecBf16; }},
      {"a 1x1", 1, [](ConvParams &) {}},
      {"the stem", 7, [](ConvParams &) {}},
      {"pad 0", 3, [](ConvParams &p) { p.pad = 0; }},
      {"stride 3", 3, [](ConvParams &p) { p.stride = 3; }},
      {"unsegmented", 3, [](ConvParams &p) { p.kseg_len = 0; }},
      {"a shift", 3, [](ConvParams &p) { p.T = 8; p.fold = 32; }},
      {"a residual", 3, [](ConvParams &p) { p.res = &g_dummy; }},
      {"a second source", 3, [](ConvParams &p) { p.x2 = &g_dummy; }},
      {"32x32 tiles", 3, [](ConvParams &p) { p.tile = tsm::kTile32x32; }},
      {"128x128 tiles", 3, [](ConvParams &p) { p.tile = tsm::kTile128x128; }},
      {"split-K", 3, [](ConvParams &p) { p.ksplit = 1; }},
      {"72 frames", 3, [](ConvParams &p) { p.N = 72; p.M = 72 * p.Ho * p.Wo; }},
      {"8 frames", 3, [](ConvParams &p) { p.N = 8; p.M = 8 * p.Ho * p.Wo; }},
      {"M that is not N * Ho * Wo", 3, [](ConvParams &p) { p.M += 64; }},
      {"an input past 2 GB", 3, [](ConvParams &p) { p.N = 64 * 400; p.M = p.N * p.Ho * p.Wo; p.Cout = 64; }},       // 25600 x 196 x 256 x 4 = 5.1e9
      {"an output past 2 GB", 3, [](ConvParams &p) { p.N = 8192; p.M = p.N * p.Ho * p.Wo; p.Cout = 512; }},          // 8192 x 196 x 512 x 4 = 3.3e9 (input 1.6e9)
  };
  for (const Row &row : rows) {
    ConvParams p = base;
    row.edit(p);
    EXPECT(!tsm::pos_major_valid(p, row.ks), "%s must be refused", row.what);
  }
  for (int ksplit : {0, 2}) {
    ConvParams p = base;
    p.ksplit = ksplit;
    EXPECT(tsm::pos_major_valid(p, 3), "ksplit %d is valid", ksplit);
  }
  for (int stride : {1, 2}) EXPECT(tsm::pos_major_valid(layer(64, 7, 7, 512, 512, stride), 3), "stride %d is valid", stride);
  ConvParams autot = base;
  autot.tile = tsm::kTileAuto;
  EXPECT(tsm::pos_major_valid(autot, 3), "the heuristic tile of a segmented launch is 64x64");

  // conv_route: the flag where the request and the rule meet, the natural order (same tiles, same grid) anywhere else
  const tsm::ConvRoute r1 = tsm::conv_route(base, 3, 256);
  ConvParams nat = base;
  nat.pos_major = 0;
  const tsm::ConvRoute r0 = tsm::conv_route(nat, 3, 256);
  EXPECT(r1.family == tsm::kFamIgemmSeg && r1.pos_major && r0.family == tsm::kFamIgemmSeg && !r0.pos_major, "the route's flag follows the request");
  EXPECT(r1.tiles == r0.tiles && r1.grid == r0.grid && r1.ntm == r0.ntm && r1.ntn == r0.ntn && r1.bm == 64 && r1.bn == 64, "the same tiles either way");
  ConvParams n72 = layer(72, 14, 14, 256, 256, 1);
  const tsm::ConvRoute r72 = tsm::conv_route(n72, 3, 256);
  EXPECT(r72.family == tsm::kFamIgemmSeg && !r72.pos_major, "72 frames run in natural order");
  ConvParams tail = base;
  tail.ksplit = 2;
  tail.tail_from = (int)(r1.tiles / 2 / r1.ntn * r1.ntn);
  const tsm::ConvRoute rt = tsm::conv_route(tail, 3, 256);
  EXPECT(rt.family == tsm::kFamIgemmSeg && rt.pos_major, "the tail split keeps the flag");
  ConvParams sk = base;
  sk.ksplit = 1;
  const tsm::ConvRoute rs = tsm::conv_route(sk, 3, 256);
  EXPECT(rs.family == tsm::kFamIgemmSeg && !rs.pos_major, "split-K runs in natural order");
  ConvParams one = layer(128, 14, 14, 256, 256, 1);
  one.kseg_len = 0;
  EXPECT(!tsm::conv_route(one, 3, 256).pos_major, "an unsegmented launch has no such arm");

  // next_live_kstep at its edges
  EXPECT(tsm::next_live_kstep(0, 0u, 4, 36) == 36, "no live tap");
  EXPECT(tsm::next_live_kstep(-1, 0x1ffu, 4, 36) == 36 && tsm::next_live_kstep(36, 0x1ffu, 4, 36) == 36 && tsm::next_live_kstep(1 << 30, 0x1ffu, 4, 36) == 36, "outside [0, nk)");
  EXPECT(tsm::next_live_kstep(0, 0x100u, 4, 36) == 32 && tsm::next_live_kstep(0, 0x100u, 4, 18) == 18, "the last tap, and the same clipped to a segment");
  EXPECT(tsm::next_live_kstep(5, 0xffffffffu, 1, 9) == 5 && tsm::next_live_kstep(0, 0xfffffe00u, 1, 9) == 9, "bits above tap 8 are ignored");
}

// 4. live (tile, K-step) pairs over all of them at n frames
static double live_share(int n, int hi, int c, int stride) {
  const ConvParams p = layer(n, hi, hi, c, c, stride);
  const int nk = p.Kp / 32, spt = p.C / 32;
  int64_t live = 0, all = 0;
  for (int m0 = 0; m0 < p.M; m0 += 64) {
    int frame, pos;
    tsm::pos_major_row(m0, p.N, &frame, &pos);
    const unsigned mask = tsm::pos_major_tap_mask(pos, p.Wo, p.Hi, p.Wi, p.stride, p.pad);
    for (int kt = tsm::next_live_kstep(0, mask, spt, nk); kt < nk; kt = tsm::next_live_kstep(kt + 1, mask, spt, nk)) ++live;
    all += nk;
  }
  return (double)live / (double)all;
}

int main() {
  for (int stride : {1, 2})
    for (int c : {128, 256, 512}) {
      for (int hw = 1; hw <= 9; ++hw) check_shape(hw, hw, stride, c);
      check_shape(14, 14, stride, c);
      check_shape(2, 5, stride, c);   // (a frame that is not square, without an interior position)
      check_shape(6, 3, stride, c);
    }
  check_refusals();
  const struct { const char *name; int hi, c, stride; double want; } shares[] = {
      {"layer2.0.conv2", 56, 128, 2, 0.9763}, {"layer3.0.conv2", 28, 256, 2, 0.9529}, {"layer3.1-5.conv2", 14, 256, 1, 0.9070},
      {"layer4.0.conv2", 14, 512, 2, 0.9070}, {"layer4.1-2.conv2", 7, 512, 1, 0.8186}};
  for (const auto &s : shares) {
    const double got = live_share(256, s.hi, s.c, s.stride);
    printf("live share %s %.4f\n", s.name, got);
    EXPECT(std::fabs(got - s.want) < 5e-5, "%s: live share %.5f, expected %.4f", s.name, got, s.want);
  }
  if (g_fail) {
    printf("%d failure(s)\n", g_fail);
    return 1;
  }
  printf("pos major host ok\n");
  return 0;
}
