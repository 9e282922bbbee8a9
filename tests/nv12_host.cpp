// The pure-integer pieces of the NV12 tap source (csrc/tsm_host_util.h: nv12_coefficients, frame_bytes_of, nv12_pixel_rgb,
// nv12_luma_offset / nv12_chroma_offset, nv12_window_descriptor_ok), built with -fsanitize=address,undefined and run on the CPU
// by tests/test_nv12_cpu.py: the kernels inline exactly this text.
// 1. The four coefficient rows against the table of include/tsm_hip.h, and that no other pixel code has a row.
// 2. The one-pixel conversion against the float64 matrix on a fixed set of triples, the 8 corners included: within 1, black and
//    white exact.
// 3. The luma and chroma offsets at (0, 0), (h - 1, w - 1) and odd / even x, y of 2x2 and 6x4 frames: inside the frame, even,
//    one pair per 2x2 block.
// 4. Bytes per frame by pixel code, at h = w = 65534 too.
// 5. The NV12 descriptor rule: every refusal and the matching acceptance.
#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

using tsm_host::CropGeometry;
using tsm_host::Nv12Coef;

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

struct Row {
  int pixel, y_off, cy, crv, cgu, cgv, cbu;
  double kr, kb;
  bool limited;
};
static const Row kRows[4] = {{TSM_PIXEL_NV12_BT601, 16, 19077, 26149, -6419, -13320, 33050, 0.299, 0.114, true},
                             {TSM_PIXEL_NV12_BT709, 16, 19077, 29372, -3494, -8731, 34610, 0.2126, 0.0722, true},
                             {TSM_PIXEL_NV12_BT601_FULL, 0, 16384, 22970, -5638, -11700, 29032, 0.299, 0.114, false},
                             {TSM_PIXEL_NV12_BT709_FULL, 0, 16384, 25802, -3069, -7670, 30402, 0.2126, 0.0722, false}};

static void coefficients() {
  EXPECT(TSM_PIXEL_NV12_BT601 == 16 && TSM_PIXEL_NV12_BT709 == 17 && TSM_PIXEL_NV12_BT601_FULL == 18 && TSM_PIXEL_NV12_BT709_FULL == 19,
         "pixel codes");
  for (const Row &r : kRows) {
    Nv12Coef k{-1, -1, -1, -1, -1, -1};
    EXPECT(tsm_host::nv12_coefficients(r.pixel, &k), "pixel %d has no row", r.pixel);
    EXPECT(k.y_off == r.y_off && k.cy == r.cy && k.crv == r.crv && k.cgu == r.cgu && k.cgv == r.cgv && k.cbu == r.cbu,
           "pixel %d: (%d %d %d %d %d %d)", r.pixel, k.y_off, k.cy, k.crv, k.cgu, k.cgv, k.cbu);
    // ... and the row is round(x * 2^14) of the float64 matrix
    const double ys = r.limited ? 255.0 / 219.0 : 1.0, cs = r.limited ? 255.0 / 224.0 : 1.0, kg = 1.0 - r.kr - r.kb;
    const double want[5] = {ys, 2.0 * (1.0 - r.kr) * cs, -2.0 * r.kb * (1.0 - r.kb) / kg * cs, -2.0 * r.kr * (1.0 - r.kr) / kg * cs,
                            2.0 * (1.0 - r.kb) * cs};
    const int got[5] = {k.cy, k.crv, k.cgu, k.cgv, k.cbu};
    for (int i = 0; i < 5; ++i)
      EXPECT(got[i] == (int)std::floor(want[i] * 16384.0 + 0.5), "pixel %d coefficient %d: %d vs %.6f", r.pixel, i, got[i], want[i] * 16384.0);
    const int32_t words[tsm_host::kNv12CoefWords] = {k.y_off, k.cy, k.crv, k.cgu, k.cgv, k.cbu};
    const Nv12Coef back = tsm_host::nv12_coef_of(words);
    EXPECT(back.y_off == k.y_off && back.cy == k.cy && back.crv == k.crv && back.cgu == k.cgu && back.cgv == k.cgv && back.cbu == k.cbu,
           "pixel %d: the six words do not give the row back", r.pixel);
    EXPECT(tsm_host::pixel_is_nv12(r.pixel), "pixel %d", r.pixel);
  }
  for (int pixel : {INT32_MIN, -1, 0, 1, 2, 15, 20, 21, 255, INT32_MAX}) {
    Nv12Coef k{7, 7, 7, 7, 7, 7};
    EXPECT(!tsm_host::nv12_coefficients(pixel, &k) && k.y_off == 7 && k.cbu == 7 && !tsm_host::pixel_is_nv12(pixel), "pixel %d", pixel);
  }
}

static int clamp_round(double v) {
  const double f = std::floor(v + 0.5);
  return f < 0.0 ? 0 : f > 255.0 ? 255 : (int)f;
}

static void one_pixel() {
  const int values[] = {0, 1, 15, 16, 17, 64, 127, 128, 129, 200, 234, 235, 236, 240, 254, 255};     // (0 and 255: the 8 corners)
  for (const Row &r : kRows) {
    Nv12Coef k{};
    tsm_host::nv12_coefficients(r.pixel, &k);
    const double ys = r.limited ? 255.0 / 219.0 : 1.0, cs = r.limited ? 255.0 / 224.0 : 1.0, kg = 1.0 - r.kr - r.kb;
    int worst = 0;
    for (int Y : values)
      for (int U : values)
        for (int V : values) {
          int rgb[3] = {-1, -1, -1};
          tsm_host::nv12_pixel_rgb(k, Y, U, V, rgb);
          const double c = (Y - r.y_off) * ys, d = (U - 128) * cs, e = (V - 128) * cs;
          const int want[3] = {clamp_round(c + 2.0 * (1.0 - r.kr) * e),
                               clamp_round(c - 2.0 * r.kb * (1.0 - r.kb) / kg * d - 2.0 * r.kr * (1.0 - r.kr) / kg * e),
                               clamp_round(c + 2.0 * (1.0 - r.kb) * d)};
          for (int ch = 0; ch < 3; ++ch) {
            const int diff = rgb[ch] > want[ch] ? rgb[ch] - want[ch] : want[ch] - rgb[ch];
            worst = diff > worst ? diff : worst;
            EXPECT(rgb[ch] >= 0 && rgb[ch] <= 255 && diff <= 1, "pixel %d (%d %d %d) channel %d: %d vs %d", r.pixel, Y, U, V, ch, rgb[ch], want[ch]);
          }
        }
    int rgb[3];
    tsm_host::nv12_pixel_rgb(k, r.y_off, 128, 128, rgb);
    EXPECT(rgb[0] == 0 && rgb[1] == 0 && rgb[2] == 0, "pixel %d: black is (%d %d %d)", r.pixel, rgb[0], rgb[1], rgb[2]);
    tsm_host::nv12_pixel_rgb(k, r.limited ? 235 : 255, 128, 128, rgb);
    EXPECT(rgb[0] == 255 && rgb[1] == 255 && rgb[2] == 255, "pixel %d: white is (%d %d %d)", r.pixel, rgb[0], rgb[1], rgb[2]);
    tsm_host::nv12_pixel_rgb(k, 0, 0, 0, rgb);
    const int green[4] = {136, 77, 135, 84};
    EXPECT(rgb[0] == 0 && rgb[1] == green[r.pixel - 16] && rgb[2] == 0, "pixel %d: zero bytes are (%d %d %d)", r.pixel, rgb[0], rgb[1], rgb[2]);
    std::printf("pixel %d: largest |integer - float64| over %zu^3 triples: %d\n", r.pixel, sizeof values / sizeof values[0], worst);
  }
}

static void offsets_of(int h, int w) {
  const int64_t frame = tsm_host::frame_bytes_of(TSM_PIXEL_NV12_BT601, h, w);
  EXPECT(frame == (int64_t)h * w * 3 / 2, "%d x %d: %lld bytes", h, w, (long long)frame);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int64_t l = tsm_host::nv12_luma_offset(w, y, x), c = tsm_host::nv12_chroma_offset(h, w, y, x);
      EXPECT(l == (int64_t)y * w + x && l >= 0 && l < (int64_t)h * w, "%d x %d luma (%d, %d): %lld", h, w, y, x, (long long)l);
      EXPECT(c == (int64_t)h * w + (int64_t)(y / 2) * w + 2 * (x / 2), "%d x %d chroma (%d, %d): %lld", h, w, y, x, (long long)c);
      EXPECT(c % 2 == 0 && c >= (int64_t)h * w && c + 1 < frame, "%d x %d chroma (%d, %d): %lld outside the plane", h, w, y, x, (long long)c);
      EXPECT(c == tsm_host::nv12_chroma_offset(h, w, y & ~1, x & ~1) && c == tsm_host::nv12_chroma_offset(h, w, y | 1, x | 1),
             "%d x %d (%d, %d): a 2x2 block shares one pair", h, w, y, x);
    }
  EXPECT(tsm_host::nv12_chroma_offset(h, w, 0, 0) == (int64_t)h * w, "%d x %d: the first pair follows the luma plane", h, w);
  EXPECT(tsm_host::nv12_chroma_offset(h, w, h - 1, w - 1) == frame - 2, "%d x %d: the last pair ends the frame", h, w);
}

static void bytes() {
  offsets_of(2, 2);
  offsets_of(6, 4);
  offsets_of(4, 6);
  EXPECT(tsm_host::frame_bytes_of(TSM_PIXEL_U8, 5, 7) == 105 && tsm_host::frame_bytes_of(TSM_PIXEL_F32, 5, 7) == 420, "RGB frames");
  for (int pixel = 16; pixel <= 19; ++pixel) {
    EXPECT(tsm_host::frame_bytes_of(pixel, 65534, 65534) == (int64_t)65534 * 65534 / 2 * 3, "pixel %d at 65534^2", pixel);
    EXPECT(tsm_host::frame_bytes_of(pixel, 65534, 65534) == 6442057734LL, "pixel %d at 65534^2", pixel);
    EXPECT(tsm_host::frame_bytes_of(pixel, 5, 6) == -1 && tsm_host::frame_bytes_of(pixel, 6, 5) == -1, "pixel %d: an odd side", pixel);
    EXPECT(tsm_host::frame_bytes_of(pixel, 0, 2) == -1 && tsm_host::frame_bytes_of(pixel, 2, -2) == -1, "pixel %d: a non-positive side", pixel);
  }
  EXPECT(tsm_host::frame_bytes_of(TSM_PIXEL_U8, 65535, 65535) == (int64_t)65535 * 65535 * 3, "u8 at 65535^2");
  EXPECT(tsm_host::frame_bytes_of(TSM_PIXEL_F32, 65535, 65535) == (int64_t)65535 * 65535 * 12, "f32 at 65535^2");
  for (int pixel : {-1, 2, 15, 20, INT32_MAX}) EXPECT(tsm_host::frame_bytes_of(pixel, 4, 4) == -1, "pixel %d", pixel);
  EXPECT(tsm_host::nv12_chroma_offset(65534, 65534, 65533, 65533) == 6442057734LL - 2, "the last pair of a 65534^2 frame");
}

static bool ok(int64_t off, int h, int w, int n_segment, int64_t arena, bool center = false, int resize = 36, int crop = 32,
               int64_t *off_out = nullptr) {
  const uint64_t u = (uint64_t)off;
  const int32_t d[8] = {(int32_t)(uint32_t)(u & 0xFFFFFFFFu), (int32_t)(uint32_t)(u >> 32), h, w, 3, 5, 7, 9};
  int64_t o = -12345;
  CropGeometry g{-1, -1, -1, -1};
  const bool r = tsm_host::nv12_window_descriptor_ok(d, n_segment, arena, center, resize, crop, &o, &g);
  if (r) EXPECT(o == off, "offset %lld came back as %lld", (long long)off, (long long)o);
  if (r && center) {
    CropGeometry want;
    EXPECT(tsm_host::center_crop_geometry_int(h, w, resize, crop, &want) && want.nh == g.nh && want.nw == g.nw && want.top == g.top &&
               want.left == g.left, "%d x %d: geometry", h, w);
  }
  if (off_out) *off_out = o;
  return r;
}

static void descriptors() {
  const int h = 52, w = 90, t = 8;
  const int64_t frame = (int64_t)h * w * 3 / 2, win = t * frame, arena = 4096 + win;
  EXPECT(ok(0, h, w, t, arena) && ok(4096, h, w, t, arena) && ok(16, h, w, t, arena), "windows inside the arena");
  EXPECT(ok(4096, h, w, t, arena, true), "the centre crop of a 52 x 90 frame");
  EXPECT(!ok(4096, h, w, t, arena - 1), "one byte short of the arena");
  EXPECT(!ok(4096 + 16, h, w, t, arena), "16 bytes past the last fit");
  EXPECT(ok(4096, h, w, t - 1, arena - frame) && !ok(4096, h, w, t, arena - frame), "one frame short");
  for (int64_t off : {(int64_t)1, (int64_t)2, (int64_t)8, (int64_t)15, (int64_t)4095}) EXPECT(!ok(off, h, w, 1, arena), "offset %lld", (long long)off);
  EXPECT(!ok(-16, h, w, t, arena) && !ok(INT64_MIN, h, w, t, arena) && !ok(INT64_MAX - 15, h, w, t, arena) && !ok(arena + 16, 2, 2, 1, arena),
         "offsets outside the arena");
  // an odd side, where the same window with the even side below / above it fits
  EXPECT(!ok(0, 51, w, t, arena) && ok(0, 50, w, t, arena), "odd h");
  EXPECT(!ok(0, h, 89, t, arena) && ok(0, h, 88, t, arena), "odd w");
  EXPECT(!ok(0, 1, 2, 1, arena) && !ok(0, 2, 1, 1, arena) && !ok(0, 0, 2, 1, arena) && !ok(0, 2, 0, 1, arena) && ok(0, 2, 2, 1, arena),
         "the smallest frame is 2 x 2");
  EXPECT(!ok(0, -2, 2, 1, arena) && !ok(0, 2, INT32_MIN, 1, arena) && !ok(0, INT32_MAX, 2, 1, arena) && !ok(0, 65536, 2, 1, arena) &&
             !ok(0, 2, 65536, 1, arena) && !ok(0, 65535, 2, 1, INT64_MAX),
         "sides outside 2 .. 65534");
  const int64_t big = (int64_t)65534 * 65534 / 2 * 3;
  EXPECT(ok(0, 65534, 65534, 1, big) && !ok(0, 65534, 65534, 1, big - 1) && ok(16, 65534, 65534, 2, 2 * big + 16), "the largest frame");
  // n_segment * bytes leaves int64: refused, not wrapped
  EXPECT(!ok(0, 65534, 65534, INT32_MAX, INT64_MAX), "INT32_MAX frames of 65534^2");
  EXPECT(!ok(0, 65534, 65534, INT32_MAX, big), "INT32_MAX frames of 65534^2 in an arena of one");
  EXPECT(ok(0, 2, 2, INT32_MAX, (int64_t)INT32_MAX * 6) && !ok(0, 2, 2, INT32_MAX, (int64_t)INT32_MAX * 6 - 1), "INT32_MAX frames of 2 x 2");
  // the centre crop must fit the resized frame (crop > resize), and the long side must fit an int32
  EXPECT(!ok(0, h, w, t, arena, true, 32, 36) && ok(0, h, w, t, arena, false, 32, 36), "crop 36 of a frame resized to 32");
  EXPECT(!ok(0, 2, 65534, 1, arena + big, true, INT32_MAX, 1), "long side of 2^31 * 32767");
  // an RGB window and an NV12 window of one size differ in bytes: the sibling rule is untouched
  const int32_t d[8] = {0, 0, h, w, 0, 0, 0, 0};
  int64_t o;
  CropGeometry g;
  EXPECT(tsm_host::window_descriptor_ok(d, t, 1, 2 * win, false, 36, 32, &o, &g) && !tsm_host::window_descriptor_ok(d, t, 1, 2 * win - 1, false, 36, 32, &o, &g),
         "the RGB rule");
  EXPECT(tsm_host::nv12_window_descriptor_ok(d, t, win, false, 36, 32, &o, &g), "the NV12 rule at half the bytes");
}

int main() {
  coefficients();
  one_pixel();
  bytes();
  descriptors();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("nv12_host ok\n");
  return 0;
}
