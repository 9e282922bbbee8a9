// The pure-host arithmetic of the TDN engine (csrc/tsm_host_util.h: tdn_nearest, tdn_*_size, tdn_refusal, tdn_chunk_clips,
// tdn_patch_k / tdn_patch_source, tdn_pack_conv15, tdn_mean_less_bias, tdn_bn_fold, tdn_pack_mse), built with -fsanitize=address,undefined and
// run on the CPU by tests/test_tdn_cpu.py: the sizes the engine hands the kernels and the weights it uploads.
//   tdn_host
#include <cinttypes>
#include <cmath>
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
  // sides through the network: 224 -> P 112, conv1_5 56, xd0 28; trunk 56, 28, 14, 7.  96 x 160 and 64 likewise.
  const int in[4] = {224, 64, 96, 160};
  const int want[4][7] = {{112, 56, 28, 56, 28, 14, 7}, {32, 16, 8, 16, 8, 4, 2}, {48, 24, 12, 24, 12, 6, 3}, {80, 40, 20, 40, 20, 10, 5}};
  for (int i = 0; i < 4; ++i) {
    const int got[7] = {tdn_diff_pool_size(in[i]), tdn_conv15_size(in[i]), tdn_diff_size(in[i]), tdn_stage_size(in[i], 1),
                        tdn_stage_size(in[i], 2), tdn_stage_size(in[i], 3), tdn_stage_size(in[i], 4)};
    for (int k = 0; k < 7; ++k) EXPECT(got[k] == want[i][k], "side %d of input %d: %d", k, in[i], got[k]);
    EXPECT(tdn_conv15_size(in[i]) == in[i] / 4 && tdn_conv15_size(in[i]) % kTdnTile == 0, "the front end's 8 x 8 tiles partition the conv1_5 map of %d", in[i]);
  }
  EXPECT(tdn_pool_size(7) == 3 && tdn_pool_size(5) == 2 && tdn_pool_size(3) == 1 && tdn_pool_size(2) == 1, "floor-mode pool");
  // the nearest index: the identity, the doubling, 3 -> 7, 2 -> 5, 1 -> 3, and never past the end
  for (int n = 1; n <= 64; ++n)
    for (int i = 0; i < n; ++i) EXPECT(tdn_nearest(i, n, n) == i, "identity %d of %d", i, n);
  for (int i = 0; i < 56; ++i) EXPECT(tdn_nearest(i, 28, 56) == i / 2, "28 -> 56 at %d", i);
  const int up7[7] = {0, 0, 0, 1, 1, 2, 2}, up5[5] = {0, 0, 0, 1, 1};
  for (int i = 0; i < 7; ++i) EXPECT(tdn_nearest(i, 3, 7) == up7[i], "3 -> 7 at %d: %d", i, tdn_nearest(i, 3, 7));
  for (int i = 0; i < 5; ++i) EXPECT(tdn_nearest(i, 2, 5) == up5[i], "2 -> 5 at %d: %d", i, tdn_nearest(i, 2, 5));
  for (int in_n = 1; in_n <= 64; ++in_n)
    for (int out_n = 1; out_n <= 64; ++out_n)
      for (int i = 0; i < out_n; ++i) {
        const int s = tdn_nearest(i, in_n, out_n);
        EXPECT(s >= 0 && s < in_n, "nearest(%d, %d, %d) = %d", i, in_n, out_n, s);
      }
}

static void refusals() {
  using namespace tsm_host;
  const int32_t ok[4] = {3, 4, 6, 3}, zero[4] = {3, 0, 6, 3}, deep[4] = {3, 4, 65, 3}, one[4] = {1, 1, 1, 64};
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 224, 224, 0, ok) == nullptr && tdn_refusal(kPrecF32, 0, 2, 64, 96, 0, one) == nullptr, "the model and the smallest engine");
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 224, 224, 0, nullptr) != nullptr, "NULL depths");
  EXPECT(tdn_refusal(kPrecBf16, 0, 8, 224, 224, 0, ok) != nullptr && tdn_refusal(kPrecBf16x3, 0, 8, 224, 224, 0, ok) != nullptr, "fp32 only");
  EXPECT(tdn_refusal(kPrecF32, 1, 8, 224, 224, 0, ok) != nullptr, "no TSM shift");
  EXPECT(tdn_refusal(kPrecF32, 0, 1, 224, 224, 0, ok) != nullptr, "one segment");
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 32, 224, 0, ok) != nullptr && tdn_refusal(kPrecF32, 0, 8, 224, 32, 0, ok) != nullptr, "below 64");
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 200, 224, 0, ok) != nullptr && tdn_refusal(kPrecF32, 0, 8, 224, 100, 0, ok) != nullptr, "not a multiple of 32");
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 224, 224, 1, ok) != nullptr, "another topology");
  EXPECT(tdn_refusal(kPrecF32, 0, 8, 224, 224, 0, zero) != nullptr && tdn_refusal(kPrecF32, 0, 8, 224, 224, 0, deep) != nullptr, "depth range");
  // chunks: 8 clips at most, max_clips at most, and below 2^29 floats of patch rows
  EXPECT(tdn_chunk_clips(32, 8, 224, 224) == 8 && tdn_chunk_clips(3, 8, 224, 224) == 3 && tdn_chunk_clips(32, 16, 224, 224) == 8, "the usual chunks");
  EXPECT(tdn_chunk_clips(32, 8, 448, 448) == 5, "448 x 448: %d clips", tdn_chunk_clips(32, 8, 448, 448));
  EXPECT(tdn_chunk_clips(32, 8, 2048, 2048) == 0, "one clip too large: %d", tdn_chunk_clips(32, 8, 2048, 2048));
  EXPECT(tdn_chunk_clips(32, 8, INT32_MAX / 32 * 32, INT32_MAX / 32 * 32) == 0, "the largest frame");
  for (int h : {64, 224, 448, 1024}) {
    const int c = tdn_chunk_clips(32, 8, h, h);
    if (c > 0) EXPECT((int64_t)c * 8 * (h / 4) * (h / 4) * kTdnPatchK < ((int64_t)1 << 29), "chunk of %d at %d", c, h);
  }
}

static void patches() {
  using namespace tsm_host;
  std::set<int> ks;
  for (int ky = 0; ky < 7; ++ky)
    for (int kx = 0; kx < 7; ++kx)
      for (int c = 0; c < kTdnDiffC; ++c) ks.insert(tdn_patch_k(ky, kx, c));
  EXPECT((int)ks.size() == kTdnPatchReal && *ks.begin() == 0 && *ks.rbegin() == kTdnPatchReal - 1 && kTdnPatchReal == 588, "K order is a bijection onto [0, 588)");
  EXPECT(kTdnPatchK % 32 == 0 && (kTdnPatchK & (kTdnPatchK - 1)) == 0 && kTdnPatchK >= kTdnPatchReal, "K padded to a power of two");
  // every element of a patch row: a tap inside the map reads P there, a padding tap and the tail read nothing
  const int hp = 12, wp = 20, ho = 6, wo = 10;
  long reads = 0;
  for (int oy = 0; oy < ho; ++oy)
    for (int ox = 0; ox < wo; ++ox)
      for (int k = -1; k <= kTdnPatchK; ++k) {
        const int64_t src = tdn_patch_source(oy, ox, k, hp, wp);
        if (k < 0 || k >= kTdnPatchReal) {
          EXPECT(src == -1, "tail %d", k);
          continue;
        }
        const int c = k % 12, kx = k / 12 % 7, ky = k / 84, py = 2 * oy - 3 + ky, px = 2 * ox - 3 + kx;
        const bool inside = py >= 0 && py < hp && px >= 0 && px < wp;
        EXPECT(src == (inside ? ((int64_t)py * wp + px) * 12 + c : -1), "source of (%d, %d, %d)", oy, ox, k);
        EXPECT(src < (int64_t)hp * wp * 12, "inside P");
        reads += inside;
      }
  EXPECT(reads > 0, "some taps read");
  // a row of a patch is 84 contiguous floats of a [.., 21, 12] LDS tile, 16-byte aligned quads that never straddle a row
  for (int q = 0; q < kTdnPatchReal / 4; ++q) EXPECT((4 * q) / 84 == (4 * q + 3) / 84, "quad %d inside one kernel row", q);
  EXPECT(INT32_MAX / 4 > 0 && tdn_patch_source(INT32_MAX / 4, INT32_MAX / 4, 587, INT32_MAX / 2, INT32_MAX / 2) == -1, "the largest output reads padding at tap 6");
}

static void weights() {
  using namespace tsm_host;
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.5f, 1.5f);
  auto normal = [&](size_t n) { std::vector<float> v(n); for (float &x : v) x = nd(rng); return v; };
  auto bn = [&](int c) { std::vector<float> v(4 * (size_t)c); for (int i = 0; i < 4 * c; ++i) v[i] = (i / c == 0 || i / c == 3) ? ud(rng) : 0.1f * nd(rng); return v; };
  // the bias + BatchNorm fold: BN(conv + b) with the mean moved equals scale * conv + (beta + (b - mean) * scale)
  {
    const int cout = 8;
    const std::vector<float> b = bn(cout), cb = normal(cout);
    const std::vector<float> m2 = tdn_mean_less_bias(b.data() + 2 * cout, cb.data(), cout);
    for (int o = 0; o < cout; ++o) {
      const double scale = b[o] / std::sqrt((double)b[3 * cout + o] + 1e-5);
      const double want = b[cout + o] + ((double)cb[o] - b[2 * cout + o]) * scale, got = b[cout + o] - (double)m2[o] * scale;
      EXPECT(std::fabs(want - got) < 1e-6, "folded bias %d: %g vs %g", o, want, got);
    }
  }
  // conv1_5: every weight lands at its K, the tail is zero
  {
    const int cout = 64;
    const std::vector<float> w = normal((size_t)cout * 12 * 49), b = bn(cout);
    std::vector<float> wp, bias;
    tdn_pack_conv15(w.data(), b.data(), b.data() + cout, b.data() + 2 * cout, b.data() + 3 * cout, cout, &wp, &bias);
    EXPECT(wp.size() == (size_t)cout * kTdnPatchK && bias.size() == (size_t)cout, "sizes");
    for (int o = 0; o < cout; o += 9) {
      const float scale = b[o] / std::sqrt(b[3 * cout + o] + kBnEps);
      for (int k = 0; k < kTdnPatchK; ++k) {
        const float got = wp[(size_t)o * kTdnPatchK + k];
        if (k >= kTdnPatchReal) { EXPECT(got == 0.f, "tail"); continue; }
        const int c = k % 12, kx = k / 12 % 7, ky = k / 84;
        EXPECT(got == w[(((size_t)o * 12 + c) * 7 + ky) * 7 + kx] * scale, "conv1_5 weight (%d, %d)", o, k);
      }
    }
  }
  // the long-term module's packing, for the three widths
  for (int C : {128, 256, 512}) {
    const int r = C / kTdnReduction;
    const std::vector<float> c1 = normal((size_t)r * C), c2 = normal((size_t)r * 9), k2 = normal((size_t)r * r * 9), k4 = normal((size_t)r * r * 9),
                             c3 = normal((size_t)C * r), wt = normal((size_t)C * 3), b1 = bn(r), b2 = bn(r), b4 = bn(r), b3 = bn(C);
    TdnMseWeights pk;
    tdn_pack_mse(C, c1.data(), b1.data(), c2.data(), k2.data(), b2.data(), k4.data(), b4.data(), c3.data(), b3.data(), wt.data(), &pk);
    EXPECT(pk.wq.size() == (size_t)C * r && pk.bq.size() == (size_t)r && pk.dw.size() == (size_t)9 * r && pk.k2.size() == (size_t)9 * r * r &&
           pk.k4.size() == pk.k2.size() && pk.b2.size() == (size_t)r && pk.b4.size() == (size_t)r && pk.w3.size() == (size_t)C * r &&
           pk.b3.size() == (size_t)C && pk.wt.size() == (size_t)3 * C, "sizes at %d", C);
    auto scale = [](const std::vector<float> &b, int c, int o) { return b[o] / std::sqrt(b[3 * (size_t)c + o] + kBnEps); };
    for (int j = 0; j < r; ++j) {
      for (int c = 0; c < C; c += 7) EXPECT(pk.wq[(size_t)c * r + j] == c1[(size_t)j * C + c] * scale(b1, r, j), "squeeze (%d, %d)", c, j);
      EXPECT(pk.bq[j] == b1[r + j] - b1[2 * r + j] * scale(b1, r, j), "squeeze bias %d", j);
      for (int t = 0; t < 9; ++t) {
        EXPECT(pk.dw[(size_t)t * r + j] == c2[(size_t)j * 9 + t], "depthwise (%d, %d)", t, j);
        for (int i = 0; i < r; ++i) {
          EXPECT(pk.k2[((size_t)t * r + i) * r + j] == k2[((size_t)j * r + i) * 9 + t] * scale(b2, r, j), "K2 (%d, %d, %d)", t, i, j);
          EXPECT(pk.k4[((size_t)t * r + i) * r + j] == k4[((size_t)j * r + i) * 9 + t] * scale(b4, r, j), "K4 (%d, %d, %d)", t, i, j);
        }
      }
    }
    for (int c = 0; c < C; c += 5) {
      for (int i = 0; i < r; ++i) EXPECT(pk.w3[(size_t)c * r + i] == c3[(size_t)c * r + i] * scale(b3, C, c), "excite (%d, %d)", c, i);
      for (int t = 0; t < 3; ++t) EXPECT(pk.wt[(size_t)t * C + c] == wt[(size_t)c * 3 + t], "temporal (%d, %d)", t, c);
    }
  }
}

// The folds' VALUES against a fold in double, at variances where eps decides (1e-10: the root is sqrt(eps); 1e-6: eps is ten times
// the variance) and where it does not (1).  Bound: var + eps rounds once and eps itself is 1e-5 to float rounding (together at
// most 2^-24 of the scale behind the root), the root, the division and the product with a weight round once each: 4 * 2^-24;
// asserted at 8 * 2^-24 = 4.8e-7.  eps = 1.1e-5 moves the scale by 4.7 % at 1e-10 and 4.3 % at 1e-6, eps = 0 by 316 and 3.3 times.
static void fold_values() {
  using namespace tsm_host;
  const double eps = 1e-5, ulps = 8.0 / 16777216.0;
  std::mt19937 rng(11);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> ud(0.5f, 1.5f);
  for (float var0 : {1e-10f, 1e-6f, 1.0f}) {
    const int c = 64;
    std::vector<float> bn(4 * (size_t)c);
    for (int o = 0; o < c; ++o) {
      bn[o] = ud(rng) * (o % 2 ? -1.f : 1.f);
      bn[c + o] = 0.1f * nd(rng);
      bn[2 * c + o] = 0.1f * nd(rng);
      bn[3 * c + o] = var0 * ud(rng);
    }
    std::vector<float> scale, bias;
    tdn_bn_fold(bn.data(), c, &scale, &bias);
    EXPECT(scale.size() == (size_t)c && bias.size() == (size_t)c, "sizes");
    std::vector<float> w((size_t)c * kTdnDiffC * 49), wp, b15;
    for (float &x : w) x = nd(rng);
    tdn_pack_conv15(w.data(), bn.data(), bn.data() + c, bn.data() + 2 * c, bn.data() + 3 * c, c, &wp, &b15);
    for (int o = 0; o < c; ++o) {
      const double s = (double)bn[o] / std::sqrt((double)bn[3 * c + o] + eps), b = (double)bn[c + o] - (double)bn[2 * c + o] * s;
      const double b_tol = ulps * (std::fabs((double)bn[c + o]) + 2.0 * std::fabs((double)bn[2 * c + o] * s));
      EXPECT(std::isfinite(scale[o]) && std::fabs(scale[o] - s) <= ulps * std::fabs(s), "scale %d at variance %g: %.9g vs %.9g", o, var0, scale[o], s);
      EXPECT(std::isfinite(bias[o]) && std::fabs(bias[o] - b) <= b_tol, "bias %d at variance %g: %.9g vs %.9g", o, var0, bias[o], b);
      EXPECT(std::fabs(b15[o] - b) <= b_tol, "conv1_5 bias %d at variance %g: %.9g vs %.9g", o, var0, b15[o], b);
      for (int k = 0; k < kTdnPatchReal; k += 5) {
        const int ch = k % kTdnDiffC, kx = k / kTdnDiffC % 7, ky = k / (7 * kTdnDiffC);
        const double want = (double)w[(((size_t)o * kTdnDiffC + ch) * 7 + ky) * 7 + kx] * s, got = wp[(size_t)o * kTdnPatchK + tdn_patch_k(ky, kx, ch)];
        EXPECT(std::fabs(got - want) <= ulps * std::fabs(want), "conv1_5 weight (%d, %d) at variance %g: %.9g vs %.9g", o, k, var0, got, want);
      }
      // the near misses the bound must tell apart where eps decides
      if (var0 < 1e-5f)
        for (double other : {1.1e-5, 2e-5, 1e-3, 0.0}) {
          const double s2 = (double)bn[o] / std::sqrt((double)bn[3 * c + o] + other);
          EXPECT(std::fabs(s2 - s) > 1000 * ulps * std::fabs(s), "eps %g is told from 1e-5 at variance %g", other, var0);
        }
    }
  }
}

int main() {
  sizes();
  fold_values();
  refusals();
  patches();
  weights();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("tdn_host ok\n");
  return 0;
}
