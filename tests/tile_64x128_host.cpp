// The 64x128 tile (kTile64x128: conv_igemm<64, 128, 2, 2, 1, ..>, fp32 unsegmented 1x1 convs) in the launch rules of
// csrc/tsm_conv_rules.h, on the CPU under ASAN + UBSAN.  A stand-alone program (tests/test_tile_64x128_cpu.py builds and runs it):
//   1. one hand-written route per arm of the kernel (plain, shifted, residual, second source);
//   2. one row per refusal: Cout % 128 != 0, a segmented layer, a 3x3, the bf16 formats, block placement -- conv_tile_valid says
//      no (so the engine's checked_code falls back to the heuristic shape) and conv_route refuses the forced tile;
//   3. the name round trip and the tile's dimensions;
//   4. conv_tile_valid => conv_route accepts the tile with its geometry, for 1, 8 and 256 CUs over random 1x1 parameter blocks.
#include <cstdint>
#include <cstdio>
#include <random>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

static int g_fail = 0;
#define EXPECT(cond, ...)                           \
  do {                                              \
    if (!(cond)) {                                  \
      if (++g_fail <= 20) {                         \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                        \
        printf("\n");                               \
      }                                             \
    }                                               \
  } while (0)

using tsm::ConvParams;
using tsm::ConvRoute;

static float g_dummy = 0.f;

// An unsegmented fp32 k x k conv as the engine launches it: n frames of hi x wi pixels, c -> cout channels, the tile forced.
static ConvParams layer(int n, int hi, int wi, int c, int cout, int k = 1, int stride = 1, int T = 0, bool residual = false,
                        int prec = tsm::kPrecF32) {
  const tsm_host::LayerGeom g = tsm_host::layer_geometry(c, k, stride, prec);
  ConvParams p = tsm_host::conv_shape_params(g, k, stride, cout, n, hi, wi, true, T, 8, prec, residual);
  p.kseg_len = 0;
  if (residual) p.res = &g_dummy;
  p.tile = tsm::kTile64x128;
  return p;
}

struct Want { bool shift, res, dual; int ntm, ntn; };

static void expect_route(const ConvParams &p, const Want &w, int line) {
  for (int n_cu : {1, 8, 256}) {
    const ConvRoute r = tsm::conv_route(p, 1, n_cu);
    const bool ok = r.family == tsm::kFamIgemm && r.ks == 1 && r.bm == 64 && r.bn == 128 && r.wgm == 2 && r.wgn == 2 && r.shift == w.shift &&
                    r.res == w.res && r.dual == w.dual && !r.block_shift && !r.pos_major && r.ntm == w.ntm && r.ntn == w.ntn &&
                    r.tiles == (long)w.ntm * w.ntn && r.grid == (unsigned)(w.ntm * w.ntn);
    EXPECT(ok, "route of line %d at %d CUs: family %d tile %dx%d waves %dx%d arm %d%d%d%d ntm %d ntn %d tiles %ld grid %u", line, n_cu, r.family,
           r.bm, r.bn, r.wgm, r.wgn, r.shift, r.res, r.dual, r.block_shift, r.ntm, r.ntn, r.tiles, r.grid);
    EXPECT(tsm::conv_tile_valid(p, tsm::kTile64x128, n_cu), "line %d: the route accepts what conv_tile_valid refuses", line);
  }
}

static void expect_refused(const ConvParams &p, int ks, const char *what) {
  for (int n_cu : {1, 8, 256}) {
    EXPECT(tsm::conv_route(p, ks, n_cu).family == tsm::kFamInvalid, "%s: the forced tile is routed", what);
    ConvParams q = p;          // ... and the heuristic shape runs the launch on another tile
    q.tile = tsm::kTileAuto;
    const ConvRoute r = tsm::conv_route(q, ks, n_cu);
    EXPECT(r.family != tsm::kFamInvalid && !(r.bm == 64 && r.bn == 128), "%s: no fallback (family %d, %dx%d)", what, r.family, r.bm, r.bn);
  }
}

static void arms() {
  // layer3.1-5.conv3 of the headline: 256 frames of 14x14, 256 -> 1024 with the residual
  expect_route(layer(256, 14, 14, 256, 1024, 1, 1, 0, true), Want{false, true, false, 784, 8}, __LINE__);
  // layer2.1-3.conv1: 28x28, 512 -> 128 through the shift
  expect_route(layer(256, 28, 28, 512, 128, 1, 1, 8), Want{true, false, false, 3136, 1}, __LINE__);
  // plain, 75 rows: the second row tile is partial
  expect_route(layer(3, 5, 5, 64, 256), Want{false, false, false, 2, 2}, __LINE__);
  // layer2.0.conv3 + downsample: 128 channels at 28x28 and 256 of the 56x56 block input at stride 2, K = 384
  ConvParams p = layer(256, 28, 28, 128, 512);
  tsm_host::second_source_shape(&p, 256, 256, 56, 56, 2);
  p.x2 = &g_dummy;
  EXPECT(p.kseg_len == 0 && p.Kp == 384, "K 384 is unsegmented");
  expect_route(p, Want{false, false, true, 3136, 4}, __LINE__);
}

static void refusals() {
  using namespace tsm;
  EXPECT(!conv_tile_valid(layer(3, 5, 5, 64, 192), kTile64x128, 256), "Cout 192");
  expect_refused(layer(3, 5, 5, 64, 192), 1, "Cout 192");
  ConvParams seg = layer(3, 5, 5, 1024, 128);     // a segmented layer (layer3.1-5.conv1's K)
  seg.kseg_len = tsm_host::layer_geometry(1024, 1, 1, kPrecF32).kseg;
  EXPECT(seg.kseg_len > 0 && !conv_tile_valid(seg, kTile64x128, 256), "segmented");
  expect_refused(seg, 1, "segmented");
  EXPECT(!conv_tile_valid(layer(3, 5, 5, 32, 128, 3), kTile64x128, 256), "3x3");
  expect_refused(layer(3, 5, 5, 32, 128, 3), 3, "3x3");
  ConvParams odd = layer(3, 5, 5, 64, 128);       // a 1x1's parameter block behind ks = 3: conv_tile_valid has no ks, the route has
  EXPECT(conv_tile_valid(odd, kTile64x128, 256) && conv_route(odd, 3, 256).family == kFamInvalid, "ks 3 without padding");
  for (int prec : {(int)kPrecBf16x3, (int)kPrecBf16}) {
    EXPECT(!conv_tile_valid(layer(3, 5, 5, 64, 128, 1, 1, 0, false, prec), kTile64x128, 256), "prec %d", prec);
    expect_refused(layer(3, 5, 5, 64, 128, 1, 1, 0, false, prec), 1, "bf16 formats");
  }
  // block placement: T > 0 shifts the identity (residual / second source) or the input of a 1x1 at stride 2
  ConvParams bres = layer(8, 5, 5, 64, 128, 1, 1, 8, true);
  bres.fold = 128 / 8;
  EXPECT(!conv_tile_valid(bres, kTile64x128, 256), "shifted residual");
  expect_refused(bres, 1, "shifted residual");
  ConvParams bdual = layer(8, 3, 3, 64, 128);
  tsm_host::second_source_shape(&bdual, 32, 32, 6, 6, 2);
  bdual.x2 = &g_dummy; bdual.T = 8; bdual.fold = 32 / 8;
  EXPECT(!conv_tile_valid(bdual, kTile64x128, 256), "shifted second source");
  expect_refused(bdual, 1, "shifted second source");
  ConvParams bs2 = layer(8, 6, 6, 64, 128, 1, 2, 8);
  EXPECT(!conv_tile_valid(bs2, kTile64x128, 256), "shifted 1x1 at stride 2");
  expect_refused(bs2, 1, "shifted 1x1 at stride 2");
}

static void names() {
  using namespace tsm;
  EXPECT(kTile64x128 == 9 && kNumTiles == 10, "tile code");
  EXPECT(conv_tile_from_name("64x128") == kTile64x128, "name");
  EXPECT(conv_tile_from_name("64x128 ") == kTileAuto && conv_tile_from_name("128x64") == kTile128x64, "neighbours of the name");
  int bm = 0, bn = 0;
  conv_tile_dims(kTile64x128, &bm, &bn);
  EXPECT(bm == 64 && bn == 128, "dims %dx%d", bm, bn);
  EXPECT((kTile64x128 & tsm_host::kCodeTileMask) == kTile64x128 && (kTile64x128 & ~tsm_host::kCodeValid) == 0, "the code fits the tile mask");
}

// Random 1x1 parameter blocks (every form the engine and the per-op entry build, and some they do not): wherever conv_tile_valid
// offers the tile and the launch's arguments are not refused as such, the route accepts it with the tile's geometry.
static void fuzz(unsigned seed, int rounds) {
  std::mt19937 rng(seed);
  auto pick = [&rng](std::initializer_list<int> v) { return v.begin()[rng() % v.size()]; };
  long offered = 0, accepted = 0;
  for (int i = 0; i < rounds; ++i) {
    const int prec = pick({0, 0, 0, 1, 2}), c = pick({32, 64, 128, 256, 512, 1024, 2048}), cout = pick({64, 128, 192, 256, 512, 1024});
    const int stride = pick({1, 1, 2}), T = pick({0, 0, 8, 3}), n = pick({1, 3, 8, 24, 256});
    const bool residual = rng() % 4 == 0;
    ConvParams p = layer(n, pick({1, 5, 6, 7, 14, 28}), pick({1, 5, 6, 7, 14, 28}), c, cout, 1, stride, T, residual, prec);
    if (rng() % 4 == 0) p.kseg_len = tsm_host::layer_geometry(c, 1, stride, prec).kseg;
    if (rng() % 4 == 0) {
      const int c2 = pick({32, 64, 256}), s2 = pick({1, 2});
      tsm_host::second_source_shape(&p, c2, c2, p.Ho * s2, p.Wo * s2, s2);
      if (rng() % 2) p.kseg_len = 0;
      p.x2 = &g_dummy;
    }
    if (rng() % 8 == 0) p.pad = 1;
    p.reverse = (int)(rng() & 1);
    for (int n_cu : {1, 8, 256}) {
      if (!tsm::conv_tile_valid(p, tsm::kTile64x128, n_cu)) continue;
      ++offered;
      const ConvRoute r = tsm::conv_route(p, 1, n_cu);
      if (tsm::conv_args_refused(p, 1)) {
        EXPECT(r.family == tsm::kFamInvalid, "round %d: refused arguments are routed", i);
        continue;
      }
      ++accepted;
      EXPECT(r.family == tsm::kFamIgemm && r.bm == 64 && r.bn == 128 && r.wgm == 2 && r.wgn == 2 && !r.block_shift && !r.pos_major,
             "round %d: family %d tile %dx%d", i, r.family, r.bm, r.bn);
      EXPECT((long)r.ntm * 64 >= p.M && (long)(r.ntm - 1) * 64 < p.M && r.ntn * 128 == p.Cout && r.tiles == (long)r.ntm * r.ntn &&
             (long)r.grid == r.tiles, "round %d: ntm %d ntn %d tiles %ld grid %u for M %d Cout %d", i, r.ntm, r.ntn, r.tiles, r.grid, p.M, p.Cout);
      EXPECT(p.prec == tsm::kPrecF32 && p.pad == 0 && p.kseg_len == 0 && p.Cout % 128 == 0 && !(p.T > 0 && (p.res || p.x2 || p.stride != 1)),
             "round %d: offered outside the arm's forms", i);
      EXPECT(r.shift == (p.T > 0) && r.res == (p.res != nullptr) && r.dual == (p.x2 != nullptr), "round %d: arm %d%d%d", i, r.shift, r.res, r.dual);
    }
  }
  EXPECT(offered > rounds / 20 && accepted > offered / 2, "the loop is vacuous: %ld offered, %ld accepted of %d", offered, accepted, rounds);
  printf("64x128: offered for %ld of %d random 1x1 blocks x 3 CU counts, %ld routed\n", offered, rounds, accepted);
}

int main() {
  arms();
  refusals();
  names();
  fuzz(64128u, 20000);
  if (g_fail) {
    printf("%d failure(s)\n", g_fail);
    return 1;
  }
  printf("tile 64x128 host ok\n");
  return 0;
}
