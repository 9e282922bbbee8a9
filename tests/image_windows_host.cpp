// The pure-integer pieces of tsm_preprocess_windows' image mode (csrc/tsm_host_util.h: image_ksize_int, image_rows_cap_int,
// image_band and image_window_ok), built with -fsanitize=address,undefined and run on the CPU by tests/test_image_stream_cpu.py
// BEFORE the kernel that inlines them ever runs on a GPU: they are the kernel's geometry and its bounds logic.
//   image_windows_host <geometry.bin>
// 1. For every h, w in 1 .. 300 and (resize, crop) in {(256, 224), (24, 16), (16, 15), (8, 8)}: the window {0, 0, h, w, 0, 0}
//    in an arena that is large enough; a record (h, w, resize, crop, ok, nh, nw, top, left, ksx, ksy, words as int32) goes to
//    <geometry.bin>, where the Python test compares it with transform.resized_hw, Python's round, pil_ksize and
//    image_tables(...).size.  Here: the row cap is never below the launcher's double rule, and the band is the first that fits.
// 2. image_window_ok's verdicts: the edge words by hand, then random words against a 128-bit restatement of the rule.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

using tsm_host::ImageWindow;

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

static const int kPairs[4][2] = {{256, 224}, {24, 16}, {16, 15}, {8, 8}};
static const int kLds = 65536;

struct Desc {
  int32_t d[8];
};
static Desc desc(int64_t off, int32_t h, int32_t w, int64_t tab = 0, int32_t r6 = 0, int32_t r7 = 0) {
  return Desc{{(int32_t)(uint32_t)((uint64_t)off & 0xFFFFFFFFu), (int32_t)(off >> 32), h, w,
               (int32_t)(uint32_t)((uint64_t)tab & 0xFFFFFFFFu), (int32_t)(tab >> 32), r6, r7}};
}

// the launcher's rule of tsm_preprocess_image (image_rows_cap), in double
static int rows_cap_double(int band, int in, int out) {
  const double scale = (double)in / out, support = scale < 1.0 ? 1.0 : scale;
  return (int)((band - 1) * scale + 2.0 * support) + 2;
}

static void geometry(std::FILE *out) {
  for (const auto &rc : kPairs)
    for (int h = 1; h <= 300; ++h)
      for (int w = 1; w <= 300; ++w) {
        const Desc x = desc(0, h, w, 0);
        ImageWindow win{};
        const bool ok = tsm_host::image_window_ok(x.d, 1, false, (int64_t)1 << 40, rc[0], rc[1], kLds, &win);
        int32_t rec[12] = {h, w, rc[0], rc[1], ok, 0, 0, 0, 0, 0, 0, 0};
        if (ok) {
          rec[5] = win.g.nh; rec[6] = win.g.nw; rec[7] = win.g.top; rec[8] = win.g.left; rec[9] = win.ksx; rec[10] = win.ksy;
          rec[11] = (int32_t)(win.hwords + win.vwords);
          EXPECT(win.off == 0 && win.tab == 0, "%d x %d: offsets", h, w);
          // the band: the largest of 8, 4, 2, 1 whose rows fit, its cap at least the double rule's
          const int stride = tsm_host::image_row_stride(rc[1]);
          EXPECT(win.band == 8 || win.band == 4 || win.band == 2 || win.band == 1, "%d x %d: band %d", h, w, win.band);
          EXPECT((int64_t)win.rows_cap * stride <= kLds, "%d x %d: %d rows of %d bytes", h, w, win.rows_cap, stride);
          if (win.ksy) {
            EXPECT(win.rows_cap >= rows_cap_double(win.band, h, win.g.nh) && win.rows_cap <= rows_cap_double(win.band, h, win.g.nh) + 1,
                   "%d x %d band %d: cap %d, the double rule %d", h, w, win.band, win.rows_cap, rows_cap_double(win.band, h, win.g.nh));
            if (win.band < 8)
              EXPECT((int64_t)tsm_host::image_rows_cap_int(2 * win.band, h, win.g.nh) * stride > kLds, "%d x %d: band %d though %d fits", h, w,
                     win.band, 2 * win.band);
          } else {
            EXPECT(win.band == 8 && win.rows_cap == 8, "%d x %d: no vertical pass, band %d cap %d", h, w, win.band, win.rows_cap);
          }
        }
        if (out) std::fwrite(rec, sizeof rec, 1, out);
      }
  // the tap count at the ends of the range: ceil in integers
  EXPECT(tsm_host::image_ksize_int(65535, 1) == 2 * 65535 + 1, "ksize 65535 -> 1");
  EXPECT(tsm_host::image_ksize_int(1, INT32_MAX) == 3, "ksize 1 -> INT32_MAX");
  EXPECT(tsm_host::image_ksize_int(65535, INT32_MAX) == 3, "ksize 65535 -> INT32_MAX");
  EXPECT(tsm_host::image_ksize_int(257, 256) == 5 && tsm_host::image_ksize_int(512, 256) == 5 && tsm_host::image_ksize_int(513, 256) == 7, "ksize around 2");
  EXPECT(tsm_host::image_row_stride(tsm_host::kImageMaxCrop) == 65536 && tsm_host::image_row_stride(15) == 48, "row stride");
}

// the rule of include/tsm_hip.h restated in 128 bits
static bool want_ok(const int32_t d[8], int n_segment, bool nv12, int64_t arena_bytes, int resize, int crop, int lds) {
  typedef __int128 i128;
  const i128 off = (i128)d[1] * ((i128)1 << 32) + (uint32_t)d[0];
  const i128 h = d[2], w = d[3];
  if (off < 0 || off % 16 != 0) return false;
  if (h < 1 || h > 65535 || w < 1 || w > 65535) return false;
  if (nv12 && (h % 2 != 0 || w % 2 != 0)) return false;
  const i128 frame = nv12 ? h * w * 3 / 2 : h * w * 3;
  if (off + (i128)n_segment * frame > (i128)arena_bytes) return false;
  const i128 lng = h <= w ? (i128)resize * w / h : (i128)resize * h / w;
  if (crop > resize || crop > lng || lng > INT32_MAX) return false;
  const i128 nh = h <= w ? resize : lng, nw = h <= w ? lng : resize;
  i128 words = 0;
  if (nw != w) { i128 c = (w + nw - 1) / nw; if (c < 1) c = 1; words += (i128)crop * (2 + 2 * c + 1); }
  i128 ky = 0;
  if (nh != h) { i128 c = (h + nh - 1) / nh; if (c < 1) c = 1; ky = 2 * c + 1; words += (i128)crop * (2 + ky); }
  if (words > 0) {
    const i128 tab = (i128)d[5] * ((i128)1 << 32) + (uint32_t)d[4];
    if (tab < 0 || tab % 16 != 0 || tab + 4 * words > (i128)arena_bytes) return false;
  }
  // one output row: (band - 1) * scale + 2 * max(scale, 1) + 2 rows at band 1, floored; its own row without a vertical pass
  const i128 stride = ((i128)crop * 3 + 3) / 4 * 4;
  const i128 rows = ky == 0 ? 1 : (h >= nh ? 2 * h / nh + 2 : 4);
  return rows * stride <= lds;
}

static bool verdict(const Desc &x, int n_segment, bool nv12, int64_t arena_bytes, int resize, int crop, ImageWindow *w = nullptr, int lds = kLds) {
  ImageWindow win{};
  const bool ok = tsm_host::image_window_ok(x.d, n_segment, nv12, arena_bytes, resize, crop, lds, &win);
  const bool want = want_ok(x.d, n_segment, nv12, arena_bytes, resize, crop, lds);
  EXPECT(ok == want, "{%d %d %d %d %d %d %d %d} n_segment %d nv12 %d arena %" PRId64 " resize %d crop %d lds %d: %d, the rule says %d", x.d[0],
         x.d[1], x.d[2], x.d[3], x.d[4], x.d[5], x.d[6], x.d[7], n_segment, (int)nv12, arena_bytes, resize, crop, lds, (int)ok, (int)want);
  if (w) *w = win;
  return ok;
}

static void validity() {
  const int T = 2, H = 40, W = 56, R = 24, C = 16;            // 40 x 56 -> 24 x 33: both axes resampled, ksx = ksy = 5
  const int64_t arena = 1 << 20, bytes = (int64_t)T * H * W * 3, words = 2 * C * (2 + 5);
  const int32_t edge[3] = {INT32_MIN, INT32_MAX, 0};
  ImageWindow win;
  for (int nv12 = 0; nv12 < 2; ++nv12) {
    for (int32_t e : edge) {
      const Desc x{{e, e, e, e, e, e, e, e}};
      EXPECT(!verdict(x, T, nv12, arena, R, C), "every word %d", e);
    }
    // one edge value in one word of a valid descriptor: the offsets' words pass as 0 (they are 0), the reserved words always
    for (int word = 0; word < 8; ++word)
      for (int32_t e : edge) {
        Desc x = desc(0, H, W, 16384, 5, 7);
        x.d[word] = e;
        const bool want = word >= 6 || ((word <= 1 || word == 5) && e == 0) || (word == 4 && e == 0);
        EXPECT(verdict(x, T, nv12, arena, R, C) == want, "word %d = %d", word, e);
      }
  }
  EXPECT(verdict(desc(0, H, W, 16384), T, false, arena, R, C, &win) && win.off == 0 && win.tab == 16384 && win.g.nh == 24 && win.g.nw == 33 &&
             win.ksx == 5 && win.ksy == 5 && win.hwords == C * 7 && win.vwords == C * 7 && win.band == 8,
         "40 x 56 at 24 / 16: %d %d ks %d %d band %d", win.g.nh, win.g.nw, win.ksx, win.ksy, win.band);
  // frame offsets
  EXPECT(verdict(desc(arena - bytes, H, W, 0), T, false, arena, R, C, &win) && win.off == arena - bytes, "the last window that fits");
  EXPECT(!verdict(desc(-16, H, W, 0), T, false, arena, R, C), "offset -16");
  EXPECT(!verdict(desc(arena, H, W, 0), T, false, arena, R, C), "offset = arena_bytes");
  EXPECT(!verdict(desc(arena - bytes + 1, H, W, 0), T, false, arena, R, C), "one byte past the last fit");
  EXPECT(!verdict(desc(arena - bytes + 16, H, W, 0), T, false, arena, R, C), "one aligned step past the last fit");
  EXPECT(!verdict(desc(8, H, W, 0), T, false, arena, R, C), "unaligned off");
  EXPECT(!verdict(desc(INT64_MAX - 15, H, W, 0), T, false, INT64_MAX, R, C), "the largest aligned offset in the largest arena");
  // table offsets
  EXPECT(verdict(desc(0, H, W, arena - 4 * words), T, false, arena, R, C, &win) && win.tab == arena - 4 * words, "the last block that fits");
  EXPECT(!verdict(desc(0, H, W, arena - 4 * words + 16), T, false, arena, R, C), "a block one aligned step late");
  EXPECT(verdict(desc(0, H, W, bytes / T), 1, false, bytes / T + 4 * words, R, C), "a block that ends with the arena");
  EXPECT(!verdict(desc(0, H, W, bytes / T), 1, false, bytes / T + 4 * words - 4, R, C), "a block that ends one word past the arena");
  EXPECT(!verdict(desc(0, H, W, -16), T, false, arena, R, C), "tab -16");
  EXPECT(!verdict(desc(0, H, W, arena), T, false, arena, R, C), "tab = arena_bytes");
  EXPECT(!verdict(desc(0, H, W, 8), T, false, arena, R, C), "unaligned tab");
  EXPECT(!verdict(desc(0, H, W, 16388), T, false, arena, R, C), "tab 16388: not a multiple of 16");
  EXPECT(!verdict(desc(0, H, W, INT64_MAX - 15), T, false, INT64_MAX, R, C), "the largest aligned tab in the largest arena");
  EXPECT(!verdict(desc(0, H, W, INT64_MIN), T, false, arena, R, C), "tab INT64_MIN");
  EXPECT(verdict(desc(0, H, W, (int64_t)1 << 32), T, false, ((int64_t)1 << 32) + 4 * words, R, C, &win) && win.tab == (int64_t)1 << 32, "a tab that needs tab_hi");
  // no tables: tab is not looked at
  EXPECT(verdict(desc(0, 24, 24, -7), T, false, arena, R, C, &win) && win.ksx == 0 && win.ksy == 0 && win.hwords + win.vwords == 0 && win.tab == 0,
         "24 x 24 at resize 24: no block, tab garbage");
  EXPECT(verdict(desc(0, 24, 41, 32), T, false, arena, R, C, &win) && win.ksx == 0 && win.ksy == 0, "24 x 41 at resize 24: Resize keeps both sides");
  // sides
  EXPECT(!verdict(desc(0, 65536, W, 0), 1, false, (int64_t)1 << 40, R, C), "h 65536");
  EXPECT(!verdict(desc(0, H, 65536, 0), 1, false, (int64_t)1 << 40, R, C), "w 65536");
  EXPECT(!verdict(desc(0, 0, W, 0), 1, false, arena, R, C) && !verdict(desc(0, -1, W, 0), 1, false, arena, R, C), "h 0, h -1");
  EXPECT(!verdict(desc(0, 41, 56, 16384), 1, true, arena, R, C) && !verdict(desc(0, 40, 57, 16384), 1, true, arena, R, C), "odd NV12 sides");
  EXPECT(verdict(desc(0, 40, 56, 16384), 1, true, arena, R, C) && verdict(desc(0, 41, 57, 16384), 1, false, arena, R, C), "... even ones, and odd RGB ones");
  EXPECT(verdict(desc(0, 40, 56, 16384), 1, true, 16384 + 4 * words, R, C) && !verdict(desc(16, 40, 56, 16384), 1, true, 40 * 56 * 3 / 2 + 15, R, C),
         "an NV12 frame is 3 h w / 2 bytes");
  EXPECT(!verdict(desc(0, H, W, 16384), T, false, arena, 16, 17), "crop 17 of a frame resized to 16");
  EXPECT(!verdict(desc(0, 65535, 1, 16384), 1, false, arena, INT32_MAX, 1), "resized long side leaves int32");
  // the LDS.  Resize(int) keeps the aspect ratio, so a vertical downscale of s needs BOTH sides s times the resized ones: 3700 x
  // 3700 at 24 / 16 (9 * 154.2 + 2 rows of 48 bytes) falls back below a band of 8, 16800 x 16800 (2 * 700 + 2 rows) does not fit
  // one row's support; 3700 x 24 and 16800 x 24 keep both sides (the short one is the resize) and are copied
  EXPECT(verdict(desc(0, 3700, 3700, (int64_t)1 << 26), 1, false, (int64_t)1 << 27, R, C, &win) && win.band == 4 && win.ksy == 2 * 155 + 1, "3700 x 3700: band %d", win.band);
  EXPECT(!verdict(desc(0, 16800, 16800, (int64_t)1 << 30), 1, false, (int64_t)1 << 31, R, C), "16800 x 16800: one row's support beyond 64 KB");
  EXPECT(verdict(desc(0, 16320, 16320, (int64_t)1 << 30), 1, false, (int64_t)1 << 31, R, C, &win) && win.band == 1, "16320 x 16320: 2 * 680 + 2 rows, band %d", win.band);
  EXPECT(verdict(desc(0, 3700, 24, 0), 1, false, arena, R, C, &win) && win.ksy == 0 && win.band == 8, "3700 x 24 is copied");
  EXPECT(verdict(desc(0, 16800, 24, 0), 1, false, (int64_t)1 << 24, R, C, &win) && win.ksx == 0 && win.ksy == 0, "16800 x 24 is copied");
  EXPECT(!verdict(desc(0, 65535, 65535, 0), 1, false, (int64_t)1 << 40, R, C), "65535 x 65535 at 24: a downscale of 2730");
  EXPECT(verdict(desc(0, 65535, 65535, (int64_t)1 << 34), 1, false, (int64_t)1 << 40, 32768, C, &win) && win.ksx == 5 && win.band == 8, "65535 x 65535 at 32768");

  // random words, the special values mixed in, against the 128-bit rule (verdict() compares)
  std::mt19937_64 rng(20241020);
  const int32_t special[] = {INT32_MIN, INT32_MAX, 0, -1, 1, 16, -16, 15, 65535, 65536, H, W, 24, (int32_t)arena, (int32_t)(arena - bytes), 16384};
  const int n_special = (int)(sizeof special / sizeof special[0]);
  int accepted = 0;
  for (int it = 0; it < 200000; ++it) {
    Desc x;
    for (int k = 0; k < 8; ++k) {
      const uint64_t r = rng();
      x.d[k] = (r & 3) == 0 ? (int32_t)(r >> 32) : (r & 3) == 1 ? special[(r >> 8) % n_special]
                                                                 : (int32_t)((r >> 8) % (k == 2 ? 20000 : 400)) * (k == 0 || k == 4 ? 16 : 1);
    }
    if ((it & 3) != 3) x.d[1] = x.d[5] = 0;
    const uint64_t r = rng();
    const int n_segment = (r & 7) == 0 ? INT32_MAX : 1 + (int)((r >> 8) % 4);
    const int64_t ab = (r & 0x30) == 0 ? INT64_MAX : (r & 0x30) == 0x10 ? arena : 1 + (int64_t)((r >> 16) % (1 << 26));
    const int resize = 1 + (int)((r >> 40) % 300);
    const int crop = (r & 0x100) ? 1 + (int)((r >> 50) % 300) : 1 + (int)((r >> 50) % resize);
    accepted += verdict(x, n_segment, (r & 0x40) != 0, ab, resize, crop, nullptr, (r & 0x80) ? kLds : 4096);
  }
  EXPECT(accepted > 1000 && accepted < 199000, "the random descriptors exercise both verdicts: %d accepted", accepted);
}

int main(int argc, char **argv) {
  std::FILE *out = argc > 1 ? std::fopen(argv[1], "wb") : nullptr;
  if (argc > 1 && !out) {
    std::printf("cannot write %s\n", argv[1]);
    return 2;
  }
  geometry(out);
  if (out) std::fclose(out);
  validity();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("image windows host ok\n");
  return 0;
}
