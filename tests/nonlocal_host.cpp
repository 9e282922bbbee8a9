// The pure-host arithmetic of the non-local blocks (csrc/tsm_host_util.h: nonlocal_wrapped, pool2_size, nonlocal_positions,
// nonlocal_keys, tiles_over, fold_and_pack_bias), built with -fsanitize=address,undefined and run on the CPU by
// tests/test_nonlocal_cpu.py: the sizes the engine hands the attention kernel and the weights it uploads.
//   nonlocal_host
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

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
  // make_non_local: layer2.{0, 2}, layer3.{0, 2, 4} of a [3, 4, 6, 3] backbone
  int wrapped = 0;
  const int blocks[4] = {3, 4, 6, 3};
  for (int l = 1; l <= 4; ++l)
    for (int b = 0; b < blocks[l - 1]; ++b) wrapped += nonlocal_wrapped(l, b) ? 1 : 0;
  EXPECT(wrapped == 5, "%d wrapped blocks", wrapped);
  EXPECT(nonlocal_wrapped(2, 0) && nonlocal_wrapped(2, 2) && nonlocal_wrapped(3, 0) && nonlocal_wrapped(3, 2) && nonlocal_wrapped(3, 4), "the five");
  EXPECT(!nonlocal_wrapped(2, 1) && !nonlocal_wrapped(2, 3) && !nonlocal_wrapped(1, 0) && !nonlocal_wrapped(4, 0) && !nonlocal_wrapped(3, 5), "the others");
  // floor-mode pool
  const int in[8] = {0, 1, 2, 3, 5, 10, 28, INT32_MAX}, out[8] = {0, 0, 1, 1, 2, 5, 14, INT32_MAX / 2};
  for (int i = 0; i < 8; ++i) EXPECT(pool2_size(in[i]) == out[i], "pool2_size(%d) = %d", in[i], pool2_size(in[i]));
  EXPECT(pool2_size(-4) == 0, "negative size");
  // positions: the headline shapes, the suite's, the degenerate ones, the ends of int32
  EXPECT(nonlocal_positions(8, 28, 28) == 6272 && nonlocal_keys(8, 28, 28) == 1568, "224^2 layer2");
  EXPECT(nonlocal_positions(8, 14, 14) == 1568 && nonlocal_keys(8, 14, 14) == 392, "224^2 layer3");
  EXPECT(nonlocal_positions(16, 32, 32) == 16384 && nonlocal_keys(16, 32, 32) == 4096, "256^2 T = 16 layer2");
  EXPECT(nonlocal_positions(8, 5, 5) == 200 && nonlocal_keys(8, 5, 5) == 32, "5 x 5 -> 2 x 2");
  EXPECT(nonlocal_positions(8, 3, 3) == 72 && nonlocal_keys(8, 3, 3) == 8, "3 x 3 -> 1 x 1: N_k = T");
  EXPECT(nonlocal_positions(3, 4, 6) == 72 && nonlocal_keys(3, 4, 6) == 18, "T = 3, 4 x 6");
  EXPECT(nonlocal_keys(8, 1, 7) == -1 && nonlocal_keys(8, 7, 1) == -1, "a 1-pixel side pools to nothing");
  EXPECT(nonlocal_positions(0, 4, 4) == -1 && nonlocal_positions(4, -1, 4) == -1 && nonlocal_positions(4, 4, 0) == -1, "non-positive sizes");
  EXPECT(nonlocal_positions(1, 1, INT32_MAX) == INT32_MAX, "2^31 - 1 positions still fit");
  EXPECT(nonlocal_positions(2, 1 << 15, 1 << 15) == -1, "2^31 positions do not");
  EXPECT(nonlocal_positions(INT32_MAX, INT32_MAX, INT32_MAX) == -1, "the largest arguments");
  EXPECT(nonlocal_positions(INT32_MAX, 2, 1) == -1 && nonlocal_positions(1 << 16, 1 << 15, 1) == -1, "T * h alone leaves int32");
  // tiles
  EXPECT(tiles_over(1, 64) == 1 && tiles_over(64, 64) == 1 && tiles_over(65, 64) == 2 && tiles_over(6272, 64) == 98, "query tiles");
  EXPECT(tiles_over(0, 64) == 0 && tiles_over(-3, 64) == 0 && tiles_over(5, 0) == 0, "nothing to cover");
  EXPECT(tiles_over(INT32_MAX, 64) == ((int64_t)INT32_MAX + 63) / 64, "the largest row count");
}

// fold_and_pack_bias against a double restatement: rows [row0, row0 + cout) written, every other element left alone.
static void fold(int cout, int cin, int kp, int row0, int rows, bool bn, std::mt19937 &rng) {
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.6f, 1.4f);
  std::vector<float> w((size_t)cout * cin), b(cout), gamma(cout), beta(cout), mean(cout), var(cout);
  for (float &v : w) v = nd(rng);
  for (int o = 0; o < cout; ++o) { b[o] = nd(rng); gamma[o] = ud(rng); beta[o] = nd(rng); mean[o] = nd(rng); var[o] = ud(rng); }
  const float mark = -12345.f;
  std::vector<float> wp((size_t)rows * kp, mark), bias(rows, mark);
  tsm_host::fold_and_pack_bias(w.data(), b.data(), bn ? gamma.data() : nullptr, bn ? beta.data() : nullptr, bn ? mean.data() : nullptr,
                               bn ? var.data() : nullptr, cout, cin, kp, row0, &wp, &bias);
  for (int r = 0; r < rows; ++r) {
    const int o = r - row0;
    const bool mine = o >= 0 && o < cout;
    if (!mine) EXPECT(bias[r] == mark, "bias row %d outside [%d, %d) was written", r, row0, row0 + cout);
    for (int c = 0; c < kp; ++c) {
      const float got = wp[(size_t)r * kp + c];
      if (!mine || c >= cin) {
        EXPECT(got == mark, "element (%d, %d) outside the layer's block was written", r, c);
        continue;
      }
      if (!bn) {
        EXPECT(got == w[(size_t)o * cin + c], "scale 1 must copy (%d, %d) bit for bit", r, c);
      } else {
        const double s = (double)gamma[o] / std::sqrt((double)var[o] + 1e-5), want = (double)w[(size_t)o * cin + c] * s;
        EXPECT(std::fabs(got - want) <= 1e-6 * std::fabs(want) + 1e-30, "(%d, %d): %g vs %g", r, c, (double)got, want);
      }
    }
    if (!mine) continue;
    if (!bn) {
      EXPECT(bias[r] == b[o], "bias %d must be the conv bias bit for bit", r);
    } else {
      const double s = (double)gamma[o] / std::sqrt((double)var[o] + 1e-5), want = beta[o] + ((double)b[o] - mean[o]) * s;
      EXPECT(std::fabs(bias[r] - want) <= 1e-5 * (std::fabs(want) + 1.0), "bias %d: %g vs %g", r, (double)bias[r], want);
    }
  }
}

int main() {
  sizes();
  std::mt19937 rng(7);
  fold(4, 8, 32, 0, 4, false, rng);       // theta's rows of a 3-part matrix ...
  fold(4, 8, 32, 4, 12, false, rng);      // ... phi's: the middle third
  fold(4, 8, 32, 8, 12, false, rng);      // ... g's: the last third, ending at the buffer's end
  fold(5, 7, 32, 0, 5, true, rng);        // W with its BatchNorm, odd sizes
  fold(1, 1, 32, 0, 1, true, rng);
  fold(256, 512, 512, 256, 768, false, rng);   // layer2's phi at its real size
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("nonlocal_host ok\n");
  return 0;
}
