// The pure-host arithmetic of the ConvNeXt engine (csrc/tsm_host_util.h: cnx_stem_size, cnx_down_size, cnx_stage_size, cnx_s2d_k,
// cnx_stem_k, cnx_dw_tiles, cnx_frame_elems, cnx_workspace_elems, cnx_refusal, cnx_pack_stem / _down / _dw, cnx_fold_gamma), built
// with -fsanitize=address,undefined and run on the CPU by tests/test_convnext_cpu.py: the sizes the engine hands the kernels
// and the weights it uploads.
//   convnext_host
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>
#include <set>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

static int failures = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      std::printf("FAIL %s: ", #cond);           \
      std::printf(__VA_ARGS__);                  \
      std::printf("\n");                         \
      ++failures;                                \
    }                                            \
  } while (0)

static void sizes() {
  using namespace tsm_host;
  // the floors: 224 -> 56, 28, 14, 7; the suite's 64, 80, 36, 96; the smallest frame; nothing left; the end of int32
  const int in[6] = {224, 64, 80, 36, 96, 32};
  const int want[6][4] = {{56, 28, 14, 7}, {16, 8, 4, 2}, {20, 10, 5, 2}, {9, 4, 2, 1}, {24, 12, 6, 3}, {8, 4, 2, 1}};
  for (int i = 0; i < 6; ++i)
    for (int s = 0; s < 4; ++s) EXPECT(cnx_stage_size(in[i], s) == want[i][s], "cnx_stage_size(%d, %d) = %d", in[i], s, cnx_stage_size(in[i], s));
  EXPECT(cnx_stem_size(3) == 0 && cnx_stem_size(0) == 0 && cnx_stem_size(-8) == 0 && cnx_down_size(1) == 0 && cnx_down_size(-2) == 0, "nothing left");
  EXPECT(cnx_stem_size(7) == 1 && cnx_down_size(5) == 2 && cnx_stage_size(31, 3) == 0, "floor mode");
  EXPECT(cnx_stem_size(INT32_MAX) == INT32_MAX / 4 && cnx_stage_size(INT32_MAX, 3) == INT32_MAX / 32, "the largest side");
  // the K orders are bijections onto [0, 4 C) and onto the 48 non-zero slots of [0, 64)
  for (int c : {128, 256, 512}) {
    std::set<int64_t> seen;
    for (int y = 0; y < 2; ++y)
      for (int x = 0; x < 2; ++x)
        for (int ch = 0; ch < c; ++ch) seen.insert(cnx_s2d_k(y, x, ch, c));
    EXPECT((int)seen.size() == 4 * c && *seen.begin() == 0 && *seen.rbegin() == 4 * c - 1, "s2d K order of %d channels", c);
    EXPECT(cnx_s2d_k(5, 2, 3, c) == cnx_s2d_k(1, 0, 3, c) && cnx_s2d_k(1, 0, 3, c) == 2 * c + 3, "only the parity of a pixel counts");
  }
  EXPECT(cnx_s2d_k(INT32_MAX, INT32_MAX, 1023, 1024) == 3 * 1024 + 1023, "the largest pixel");
  std::set<int> taps;
  for (int ky = 0; ky < 4; ++ky)
    for (int kx = 0; kx < 4; ++kx)
      for (int c = 0; c < 4; ++c) taps.insert(cnx_stem_k(ky, kx, c));
  EXPECT((int)taps.size() == kCnxStemK && *taps.rbegin() == kCnxStemK - 1, "stem K order");
  // tiles of the depthwise kernel
  EXPECT(cnx_dw_tile(128) == 4 && cnx_dw_tile(256) == 4 && cnx_dw_tile(512) == 4 && cnx_dw_tile(1024) == 2, "tile side per width");
  EXPECT(cnx_dw_tiles(32, 56, 56, 4) == 32 * 14 * 14 && cnx_dw_tiles(1, 7, 7, 4) == 4 && cnx_dw_tiles(3, 1, 1, 4) == 3 && cnx_dw_tiles(2, 5, 9, 4) == 2 * 2 * 3, "4 x 4 tiles");
  EXPECT(cnx_dw_tiles(32, 14, 14, 2) == 32 * 49 && cnx_dw_tiles(1, 7, 7, 2) == 16 && cnx_dw_tiles(3, 1, 1, 2) == 3 && cnx_dw_tiles(2, 5, 2, 2) == 2 * 3, "2 x 2 tiles");
  EXPECT(cnx_dw_tiles(0, 4, 4, 4) == -1 && cnx_dw_tiles(1, 0, 4, 4) == -1 && cnx_dw_tiles(1, 4, -1, 4) == -1 && cnx_dw_tiles(1, 4, 4, 0) == -1, "non-positive sizes");
  EXPECT(cnx_dw_tiles(1, INT32_MAX, 1, 4) == ((int64_t)INT32_MAX + 3) / 4 && cnx_dw_tiles(1, INT32_MAX, 1, 2) == ((int64_t)INT32_MAX + 1) / 2, "one column of the largest height");
  EXPECT(cnx_dw_tiles(INT32_MAX, INT32_MAX, INT32_MAX, 2) == -1 && cnx_dw_tiles(1 << 20, 1 << 8, 1 << 8, 4) == -1, "2^31 tiles do not fit the grid");
  EXPECT(cnx_dw_tiles((1 << 19) - 1, 1 << 8, 1 << 8, 4) == (((int64_t)1 << 19) - 1) * 64 * 64, "just below");
  // workspace
  EXPECT(cnx_frame_elems(224, 224) == (int64_t)56 * 56 * 512 && cnx_frame_elems(36, 96) == (int64_t)9 * 24 * 512 && cnx_frame_elems(3, 224) == 0, "per frame");
  EXPECT(cnx_workspace_elems(32, 224, 224) == (int64_t)32 * 56 * 56 * 512, "32 frames of 224^2");
  EXPECT(cnx_workspace_elems(0, 224, 224) == -1 && cnx_workspace_elems(4, 2, 2) == -1 && cnx_workspace_elems(-1, 64, 64) == -1, "nothing to hold");
  EXPECT(cnx_workspace_elems(334, 224, 224) == (int64_t)334 * 56 * 56 * 512 && cnx_workspace_elems(335, 224, 224) == -1, "2^29 floats is the limit");
  EXPECT(cnx_workspace_elems(INT32_MAX, INT32_MAX, INT32_MAX) == -1 && cnx_workspace_elems(1, INT32_MAX, INT32_MAX) == -1, "the largest arguments");
  EXPECT(cnx_frame_elems(INT32_MAX, INT32_MAX) == kInt31 && cnx_frame_elems(1 << 13, 1 << 13) == kInt31 && cnx_frame_elems(1 << 12, 1 << 12) == (int64_t)1 << 29, "saturates at 2^31");
}

static void refusals() {
  using namespace tsm_host;
  const int32_t base[4] = {3, 3, 27, 3}, shallow[4] = {1, 1, 2, 1}, zero[4] = {3, 0, 27, 3}, deep[4] = {3, 3, 65, 3}, neg[4] = {-1, 3, 27, 3};
  EXPECT(cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, base) == nullptr && cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, shallow) == nullptr, "accepted");
  EXPECT(cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, nullptr) != nullptr, "NULL depths");
  EXPECT(cnx_refusal(kPrecF32, 0, 8, 0, 0, 0, base) != nullptr && cnx_refusal(kPrecF32, 0, 0, 0, 0, 0, base) != nullptr, "num_segments != 1");
  EXPECT(cnx_refusal(kPrecF32, 1, 1, 0, 0, 0, base) != nullptr, "is_shift");
  EXPECT(cnx_refusal(kPrecBf16x3, 0, 1, 0, 0, 0, base) != nullptr && cnx_refusal(kPrecBf16, 0, 1, 0, 0, 0, base) != nullptr, "dtype");
  EXPECT(cnx_refusal(kPrecF32, 0, 1, 1, 0, 0, base) != nullptr && cnx_refusal(kPrecF32, 0, 1, 0, 1, 0, base) != nullptr &&
             cnx_refusal(kPrecF32, 0, 1, 0, 0, 1, base) != nullptr, "after another setter");
  EXPECT(cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, zero) != nullptr && cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, deep) != nullptr &&
             cnx_refusal(kPrecF32, 0, 1, 0, 0, 0, neg) != nullptr, "depths outside 1 .. 64");
}

// The packers against their definitions: every destination element is the one source element of its (o, c, ky, kx), the rest zero.
static void packing(std::mt19937 &rng) {
  using namespace tsm_host;
  std::normal_distribution<float> nd(0.f, 1.f);
  {
    const int cout = 5;
    std::vector<float> w((size_t)cout * 3 * 16), wp;
    for (float &v : w) v = nd(rng);
    cnx_pack_stem(w.data(), cout, &wp);
    EXPECT(wp.size() == (size_t)cout * kCnxStemK, "stem size");
    for (int o = 0; o < cout; ++o)
      for (int ky = 0; ky < 4; ++ky)
        for (int kx = 0; kx < 4; ++kx)
          for (int c = 0; c < 4; ++c) {
            const float want = c < 3 ? w[(((size_t)o * 3 + c) * 4 + ky) * 4 + kx] : 0.f;
            EXPECT(wp[(size_t)o * kCnxStemK + (ky * 4 + kx) * 4 + c] == want, "stem (%d, %d, %d, %d)", o, ky, kx, c);
          }
  }
  for (int cin : {3, 32}) {
    const int cout = 7;
    std::vector<float> w((size_t)cout * cin * 4), wp;
    for (float &v : w) v = nd(rng);
    cnx_pack_down(w.data(), cout, cin, &wp);
    EXPECT(wp.size() == (size_t)cout * 4 * cin, "downsample size");
    for (int o = 0; o < cout; ++o)
      for (int ky = 0; ky < 2; ++ky)
        for (int kx = 0; kx < 2; ++kx)
          for (int c = 0; c < cin; ++c)
            EXPECT(wp[(size_t)o * 4 * cin + (ky * 2 + kx) * cin + c] == w[(((size_t)o * cin + c) * 2 + ky) * 2 + kx], "down (%d, %d, %d, %d)", o, ky, kx, c);
  }
  {
    const int c = 12;
    std::vector<float> w((size_t)c * 49), wp;
    for (float &v : w) v = nd(rng);
    cnx_pack_dw(w.data(), c, &wp);
    EXPECT(wp.size() == (size_t)49 * c, "depthwise size");
    for (int ch = 0; ch < c; ++ch)
      for (int ky = 0; ky < 7; ++ky)
        for (int kx = 0; kx < 7; ++kx) EXPECT(wp[(size_t)(ky * 7 + kx) * c + ch] == w[((size_t)ch * 7 + ky) * 7 + kx], "dw (%d, %d, %d)", ch, ky, kx);
  }
  {
    const int cout = 6, k = 24;
    std::vector<float> w((size_t)cout * k), b(cout), g(cout), wp, bias;
    for (float &v : w) v = nd(rng);
    for (int o = 0; o < cout; ++o) { b[o] = nd(rng); g[o] = o == 2 ? 0.f : o == 3 ? 1.f : nd(rng); }
    cnx_fold_gamma(w.data(), b.data(), g.data(), cout, k, &wp, &bias);
    EXPECT(wp.size() == w.size() && bias.size() == (size_t)cout, "fold size");
    for (int o = 0; o < cout; ++o) {
      EXPECT(bias[o] == b[o] * g[o], "bias %d", o);
      for (int i = 0; i < k; ++i) EXPECT(wp[(size_t)o * k + i] == w[(size_t)o * k + i] * g[o], "(%d, %d)", o, i);
      if (o == 2) EXPECT(bias[o] == 0.f && wp[(size_t)o * k] == 0.f, "gamma 0 removes the branch");
      if (o == 3) EXPECT(bias[o] == b[o] && wp[(size_t)o * k + 1] == w[(size_t)o * k + 1], "gamma 1 copies");
    }
  }
}

int main() {
  sizes();
  refusals();
  std::mt19937 rng(11);
  packing(rng);
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("convnext_host ok\n");
  return 0;
}
