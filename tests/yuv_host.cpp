// The pure-integer pieces of the I420 / YV12 / P010 / YUYV / UYVY tap sources (csrc/tsm_host_util.h: yuv_layout_of,
// yuv_coefficients, frame_bytes_of, yuv_sides_ok / yuv_frame_bytes / yuv_alignment, yuv_y_offset / yuv_u_offset / yuv_v_offset /
// yuv_group_offset, yuv_window_descriptor_ok), built with -fsanitize=address,undefined and run on the CPU by
// tests/test_yuv_cpu.py: the kernels inline exactly this text.
// 1. The code table: 32 + 4 f + c gives format f and the coefficient row of NV12 code 16 + c; no other code gives a format.
// 2. Bytes per frame by pixel code, at 65534^2 too, and each format's parity rule.
// 3. The Y / U / V offsets of every pixel of small frames against a brute-force layout: a frame is filled with a tag per byte
//    (plane, row, column) written by nested loops over the format's definition, and every pixel must land on its own tags.
// 4. Each format's descriptor rule at its edges.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

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

static const char *const kNames[5] = {"I420", "YV12", "P010", "YUYV", "UYVY"};

static void codes() {
  EXPECT(TSM_PIXEL_I420_BT601 == 32 && TSM_PIXEL_YV12_BT709 == 37 && TSM_PIXEL_P010_BT601_FULL == 42 && TSM_PIXEL_YUYV_BT709_FULL == 47 &&
             TSM_PIXEL_UYVY_BT601 == 48 && TSM_PIXEL_UYVY_BT709_FULL == 51,
         "pixel codes");
  EXPECT(tsm_host::kYuvI420 == 0 && tsm_host::kYuvYv12 == 1 && tsm_host::kYuvP010 == 2 && tsm_host::kYuvYuyv == 3 && tsm_host::kYuvUyvy == 4 &&
             tsm_host::kYuvLayouts == 5,
         "layout numbers");
  for (int f = 0; f < 5; ++f)
    for (int c = 0; c < 4; ++c) {
      const int pixel = 32 + 4 * f + c;
      EXPECT(tsm_host::yuv_layout_of(pixel) == f, "pixel %d: layout %d", pixel, tsm_host::yuv_layout_of(pixel));
      Nv12Coef k{-1, -1, -1, -1, -1, -1}, want{};
      EXPECT(tsm_host::yuv_coefficients(pixel, &k) && tsm_host::nv12_coefficients(16 + c, &want), "pixel %d has no row", pixel);
      EXPECT(k.y_off == want.y_off && k.cy == want.cy && k.crv == want.crv && k.cgu == want.cgu && k.cgv == want.cgv && k.cbu == want.cbu,
             "pixel %d: not the row of NV12 code %d", pixel, 16 + c);
      // the NV12-only functions stay NV12-only
      Nv12Coef n{7, 7, 7, 7, 7, 7};
      EXPECT(!tsm_host::pixel_is_nv12(pixel) && !tsm_host::nv12_coefficients(pixel, &n) && n.y_off == 7, "pixel %d passes for NV12", pixel);
    }
  for (int pixel : {INT32_MIN, -1, 0, 1, 2, 15, 16, 17, 18, 19, 20, 21, 31, 52, 53, 255, INT32_MAX}) {
    Nv12Coef k{7, 7, 7, 7, 7, 7};
    EXPECT(tsm_host::yuv_layout_of(pixel) == -1 && !tsm_host::yuv_coefficients(pixel, &k) && k.y_off == 7 && k.cbu == 7, "pixel %d", pixel);
  }
  for (int pixel : {20, 21, 31, 52, 255}) EXPECT(tsm_host::frame_bytes_of(pixel, 4, 4) == -1, "pixel %d has a frame size", pixel);
}

static void bytes() {
  for (int c = 0; c < 4; ++c) {
    const int i420 = 32 + c, yv12 = 36 + c, p010 = 40 + c, yuyv = 44 + c, uyvy = 48 + c;
    for (int pixel : {i420, yv12}) {
      EXPECT(tsm_host::frame_bytes_of(pixel, 4, 6) == 36 && tsm_host::frame_bytes_of(pixel, 2, 2) == 6, "pixel %d", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 65534, 65534) == 6442057734LL, "pixel %d at 65534^2", pixel);
    }
    EXPECT(tsm_host::frame_bytes_of(p010, 4, 6) == 72 && tsm_host::frame_bytes_of(p010, 2, 2) == 12, "pixel %d", p010);
    EXPECT(tsm_host::frame_bytes_of(p010, 65534, 65534) == 2 * 6442057734LL, "pixel %d at 65534^2", p010);
    for (int pixel : {i420, yv12, p010}) {
      EXPECT(tsm_host::frame_bytes_of(pixel, 5, 6) == -1 && tsm_host::frame_bytes_of(pixel, 6, 5) == -1 && tsm_host::frame_bytes_of(pixel, 5, 5) == -1,
             "pixel %d: an odd side", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 65535, 65534) == -1 && tsm_host::frame_bytes_of(pixel, 65534, 65535) == -1, "pixel %d at 65535", pixel);
    }
    for (int pixel : {yuyv, uyvy}) {
      EXPECT(tsm_host::frame_bytes_of(pixel, 4, 6) == 48 && tsm_host::frame_bytes_of(pixel, 1, 2) == 4, "pixel %d", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 5, 6) == 60 && tsm_host::frame_bytes_of(pixel, 3, 4) == 24, "pixel %d: an odd h is legal", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 6, 5) == -1 && tsm_host::frame_bytes_of(pixel, 1, 1) == -1, "pixel %d: an odd w", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 65534, 65534) == (int64_t)65534 * 65534 * 2, "pixel %d at 65534^2", pixel);
      EXPECT(tsm_host::frame_bytes_of(pixel, 65535, 65534) == (int64_t)65535 * 65534 * 2 && tsm_host::frame_bytes_of(pixel, 65534, 65535) == -1,
             "pixel %d at 65535", pixel);
    }
    for (int pixel : {i420, yv12, p010, yuyv, uyvy})
      EXPECT(tsm_host::frame_bytes_of(pixel, 0, 2) == -1 && tsm_host::frame_bytes_of(pixel, 2, 0) == -1 && tsm_host::frame_bytes_of(pixel, -2, 2) == -1 &&
                 tsm_host::frame_bytes_of(pixel, 2, -2) == -1,
             "pixel %d: a non-positive side", pixel);
  }
  EXPECT(tsm_host::yuv_alignment(tsm_host::kYuvI420) == 1 && tsm_host::yuv_alignment(tsm_host::kYuvYv12) == 1 &&
             tsm_host::yuv_alignment(tsm_host::kYuvP010) == 4 && tsm_host::yuv_alignment(tsm_host::kYuvYuyv) == 4 &&
             tsm_host::yuv_alignment(tsm_host::kYuvUyvy) == 4,
         "alignments");
  // every frame of an aligned buffer is aligned: the frame size is a multiple of the alignment for every legal size
  for (int layout = 0; layout < 5; ++layout)
    for (int h = 1; h <= 6; ++h)
      for (int w = 2; w <= 8; w += 2)
        if (tsm_host::yuv_sides_ok(layout, h, w))
          EXPECT(tsm_host::yuv_frame_bytes(layout, h, w) % tsm_host::yuv_alignment(layout) == 0, "%s %d x %d", kNames[layout], h, w);
}

// One byte of a brute-force frame: which plane's sample it is ('Y', 'U', 'V'; 'y', 'u', 'v' the ignored low byte of a P010
// word) and of which sample (row, column) of that plane.
struct Tag {
  char plane;
  int row, col;
};

// The frame as the format's definition lays it out, byte after byte.
static std::vector<Tag> brute(int layout, int h, int w) {
  std::vector<Tag> f;
  if (layout == tsm_host::kYuvI420 || layout == tsm_host::kYuvYv12) {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) f.push_back({'Y', y, x});
    for (char plane : {layout == tsm_host::kYuvI420 ? 'U' : 'V', layout == tsm_host::kYuvI420 ? 'V' : 'U'})
      for (int y = 0; y < h / 2; ++y)
        for (int x = 0; x < w / 2; ++x) f.push_back({plane, y, x});
  } else if (layout == tsm_host::kYuvP010) {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w; ++x) {
        f.push_back({'y', y, x});            // little-endian: the low byte first
        f.push_back({'Y', y, x});
      }
    for (int y = 0; y < h / 2; ++y)
      for (int x = 0; x < w / 2; ++x) {
        f.push_back({'u', y, x});
        f.push_back({'U', y, x});
        f.push_back({'v', y, x});
        f.push_back({'V', y, x});
      }
  } else {
    for (int y = 0; y < h; ++y)
      for (int x = 0; x < w / 2; ++x) {
        const Tag y0{'Y', y, 2 * x}, u{'U', y, x}, y1{'Y', y, 2 * x + 1}, v{'V', y, x};
        if (layout == tsm_host::kYuvYuyv) {
          f.push_back(y0); f.push_back(u); f.push_back(y1); f.push_back(v);
        } else {
          f.push_back(u); f.push_back(y0); f.push_back(v); f.push_back(y1);
        }
      }
  }
  return f;
}

static void offsets_of(int layout, int h, int w) {
  const std::vector<Tag> f = brute(layout, h, w);
  const int64_t frame = tsm_host::yuv_frame_bytes(layout, h, w);
  EXPECT(tsm_host::yuv_sides_ok(layout, h, w) && (int64_t)f.size() == frame && frame == tsm_host::frame_bytes_of(32 + 4 * layout, h, w),
         "%s %d x %d: %lld bytes, the layout has %zu", kNames[layout], h, w, (long long)frame, f.size());
  const bool is420 = tsm_host::yuv_is_420(layout), grouped = layout >= tsm_host::kYuvP010;
  EXPECT(is420 == (layout <= 2), "%s", kNames[layout]);
  for (int y = 0; y < h; ++y)
    for (int x = 0; x < w; ++x) {
      const int64_t oy = tsm_host::yuv_y_offset(layout, h, w, y, x), ou = tsm_host::yuv_u_offset(layout, h, w, y, x),
                    ov = tsm_host::yuv_v_offset(layout, h, w, y, x);
      EXPECT(oy >= 0 && oy < frame && ou >= 0 && ou < frame && ov >= 0 && ov < frame, "%s %d x %d (%d, %d): %lld %lld %lld outside the frame",
             kNames[layout], h, w, y, x, (long long)oy, (long long)ou, (long long)ov);
      if (oy < 0 || oy >= frame || ou < 0 || ou >= frame || ov < 0 || ov >= frame) continue;
      const int cy = is420 ? y / 2 : y, cx = x / 2;         // 4:2:2: the chroma of the pair of the SAME row
      EXPECT(f[oy].plane == 'Y' && f[oy].row == y && f[oy].col == x, "%s %d x %d (%d, %d): Y at %lld is %c(%d, %d)", kNames[layout], h, w, y, x,
             (long long)oy, f[oy].plane, f[oy].row, f[oy].col);
      EXPECT(f[ou].plane == 'U' && f[ou].row == cy && f[ou].col == cx, "%s %d x %d (%d, %d): U at %lld is %c(%d, %d)", kNames[layout], h, w, y, x,
             (long long)ou, f[ou].plane, f[ou].row, f[ou].col);
      EXPECT(f[ov].plane == 'V' && f[ov].row == cy && f[ov].col == cx, "%s %d x %d (%d, %d): V at %lld is %c(%d, %d)", kNames[layout], h, w, y, x,
             (long long)ov, f[ov].plane, f[ov].row, f[ov].col);
      // the right sharing: the partner in x, and in the 4:2:0 layouts the partners in y, have the same chroma bytes; nothing else
      EXPECT(ou == tsm_host::yuv_u_offset(layout, h, w, y, x ^ 1) && ov == tsm_host::yuv_v_offset(layout, h, w, y, x ^ 1), "%s (%d, %d): the pair",
             kNames[layout], y, x);
      if (is420)
        EXPECT(ou == tsm_host::yuv_u_offset(layout, h, w, y ^ 1, x ^ 1) && ov == tsm_host::yuv_v_offset(layout, h, w, y ^ 1, x), "%s (%d, %d): the block",
               kNames[layout], y, x);
      else if (h > 1) {
        const int yo = (y ^ 1) < h ? (y ^ 1) : y - 1;
        EXPECT(ou != tsm_host::yuv_u_offset(layout, h, w, yo, x) && ov != tsm_host::yuv_v_offset(layout, h, w, yo, x), "%s (%d, %d): rows share nothing",
               kNames[layout], y, x);
      }
      if (x + 2 < w)
        EXPECT(ou != tsm_host::yuv_u_offset(layout, h, w, y, x + 2) && ov != tsm_host::yuv_v_offset(layout, h, w, y, x + 2), "%s (%d, %d): the next pair",
               kNames[layout], y, x);
      if (grouped) {
        // the one aligned 4-byte load: inside the frame, and it holds both chroma samples (and both lumas of a packed pair)
        const int64_t g = tsm_host::yuv_group_offset(layout, h, w, y, x);
        EXPECT(g % 4 == 0 && g >= 0 && g + 4 <= frame && ou >= g && ou < g + 4 && ov >= g && ov < g + 4, "%s %d x %d (%d, %d): group %lld",
               kNames[layout], h, w, y, x, (long long)g);
        if (layout != tsm_host::kYuvP010)
          EXPECT(oy >= g && oy < g + 4 && tsm_host::yuv_y_offset(layout, h, w, y, x ^ 1) >= g && tsm_host::yuv_y_offset(layout, h, w, y, x ^ 1) < g + 4,
                 "%s (%d, %d): the pair's luma lies in its group", kNames[layout], y, x);
        else
          EXPECT(g >= (int64_t)h * w * 2 && oy < (int64_t)h * w * 2 && oy % 2 == 1 && ou == g + 1 && ov == g + 3, "P010 (%d, %d): high bytes", y, x);
      }
    }
}

static void offsets() {
  for (int layout = 0; layout < 3; ++layout)
    for (auto hw : {std::pair<int, int>{2, 2}, {2, 4}, {4, 2}, {6, 4}, {4, 6}}) offsets_of(layout, hw.first, hw.second);
  for (int layout = 3; layout < 5; ++layout)
    for (auto hw : {std::pair<int, int>{1, 2}, {3, 4}, {2, 2}, {5, 6}, {4, 6}}) offsets_of(layout, hw.first, hw.second);
  // the last bytes of the largest frames: no intermediate leaves int64 and the last sample ends the frame
  const int m = 65534;
  EXPECT(tsm_host::yuv_v_offset(tsm_host::kYuvI420, m, m, m - 1, m - 1) == 6442057734LL - 1, "I420 at 65534^2");
  EXPECT(tsm_host::yuv_u_offset(tsm_host::kYuvYv12, m, m, m - 1, m - 1) == 6442057734LL - 1, "YV12 at 65534^2");
  EXPECT(tsm_host::yuv_group_offset(tsm_host::kYuvP010, m, m, m - 1, m - 1) == 2 * 6442057734LL - 4, "P010 at 65534^2");
  EXPECT(tsm_host::yuv_group_offset(tsm_host::kYuvUyvy, 65535, m, 65534, m - 1) == (int64_t)65535 * m * 2 - 4, "UYVY at 65535 x 65534");
}

static bool ok(int layout, int64_t off, int h, int w, int n_segment, int64_t arena, bool center = false, int resize = 36, int crop = 32) {
  const uint64_t u = (uint64_t)off;
  const int32_t d[8] = {(int32_t)(uint32_t)(u & 0xFFFFFFFFu), (int32_t)(uint32_t)(u >> 32), h, w, 3, 5, 7, 9};
  int64_t o = -12345;
  CropGeometry g{-1, -1, -1, -1};
  const bool r = tsm_host::yuv_window_descriptor_ok(layout, d, n_segment, arena, center, resize, crop, &o, &g);
  if (r) EXPECT(o == off, "offset %lld came back as %lld", (long long)off, (long long)o);
  if (!r) EXPECT(o == -12345, "a refused descriptor wrote its offset");
  if (r && center) {
    CropGeometry want;
    EXPECT(tsm_host::center_crop_geometry_int(h, w, resize, crop, &want) && want.nh == g.nh && want.nw == g.nw && want.top == g.top &&
               want.left == g.left, "%d x %d: geometry", h, w);
  }
  return r;
}

static void descriptors() {
  const int h = 52, w = 90, t = 8;
  for (int L = 0; L < 5; ++L) {
    const char *name = kNames[L];
    const bool is420 = L <= 2;
    const int64_t frame = tsm_host::yuv_frame_bytes(L, h, w), win = t * frame, arena = 4096 + win;
    EXPECT(frame == (L == 2 ? 3 * h * w : is420 ? 3 * h * w / 2 : 2 * h * w), "%s frame bytes", name);
    EXPECT(ok(L, 0, h, w, t, arena) && ok(L, 4096, h, w, t, arena) && ok(L, 16, h, w, t, arena), "%s: windows inside the arena", name);
    EXPECT(ok(L, 4096, h, w, t, arena, true), "%s: the centre crop of a 52 x 90 frame", name);
    EXPECT(!ok(L, 4096, h, w, t, arena - 1), "%s: one byte short of the arena", name);          // the last byte of the arena
    EXPECT(!ok(L, 4096 + 16, h, w, t, arena), "%s: 16 bytes past the last fit", name);
    EXPECT(ok(L, 4096, h, w, t - 1, arena - frame) && !ok(L, 4096, h, w, t, arena - frame), "%s: one frame short", name);
    for (int64_t off : {(int64_t)1, (int64_t)2, (int64_t)4, (int64_t)8, (int64_t)15, (int64_t)4095})
      EXPECT(!ok(L, off, h, w, 1, arena), "%s: offset %lld", name, (long long)off);
    EXPECT(!ok(L, -16, h, w, t, arena) && !ok(L, INT64_MIN, h, w, t, arena) && !ok(L, INT64_MAX - 15, h, w, t, arena) && !ok(L, arena + 16, 2, 2, 1, arena),
           "%s: offsets outside the arena", name);
    // parity: the window with the even side below it fits
    EXPECT(!ok(L, 0, h, 89, t, arena) && ok(L, 0, h, 88, t, arena), "%s: odd w", name);
    EXPECT(ok(L, 0, 51, w, t, arena) == !is420 && ok(L, 0, 50, w, t, arena), "%s: odd h", name);
    EXPECT(ok(L, 0, 1, 2, 1, arena) == !is420 && !ok(L, 0, 2, 1, 1, arena) && !ok(L, 0, 0, 2, 1, arena) && !ok(L, 0, 2, 0, 1, arena) && ok(L, 0, 2, 2, 1, arena),
           "%s: the smallest frame", name);
    EXPECT(!ok(L, 0, -2, 2, 1, arena) && !ok(L, 0, 2, INT32_MIN, 1, arena) && !ok(L, 0, INT32_MAX, 2, 1, arena) && !ok(L, 0, 65536, 2, 1, arena) &&
               !ok(L, 0, 2, 65536, 1, arena) && !ok(L, 0, 2, 65535, 1, INT64_MAX) && ok(L, 0, 65535, 2, 1, INT64_MAX) == !is420,
           "%s: sides outside the range", name);
    const int64_t big = tsm_host::yuv_frame_bytes(L, 65534, 65534);
    EXPECT(ok(L, 0, 65534, 65534, 1, big) && !ok(L, 0, 65534, 65534, 1, big - 1) && ok(L, 16, 65534, 65534, 2, 2 * big + 16), "%s: the largest frame", name);
    // n_segment * frame bytes leaves int64: refused, not wrapped
    EXPECT(!ok(L, 0, 65534, 65534, INT32_MAX, INT64_MAX) && !ok(L, 0, 65534, 65534, INT32_MAX, big), "%s: INT32_MAX frames of 65534^2", name);
    const int64_t small = tsm_host::yuv_frame_bytes(L, 2, 2);
    EXPECT(ok(L, 0, 2, 2, INT32_MAX, (int64_t)INT32_MAX * small) && !ok(L, 0, 2, 2, INT32_MAX, (int64_t)INT32_MAX * small - 1), "%s: INT32_MAX frames of 2 x 2", name);
    EXPECT(!ok(L, 0, h, w, t, arena, true, 32, 36) && ok(L, 0, h, w, t, arena, false, 32, 36), "%s: crop 36 of a frame resized to 32", name);
    EXPECT(!ok(L, 0, 2, 65534, 1, arena + big, true, INT32_MAX, 1), "%s: long side of 2^31 * 32767", name);
  }
}

int main() {
  codes();
  bytes();
  offsets();
  descriptors();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("yuv_host ok\n");
  return 0;
}
