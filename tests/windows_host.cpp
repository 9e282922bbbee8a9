// The pure-integer pieces of tsm_preprocess_windows' kernel (csrc/tsm_host_util.h: center_crop_geometry_int and
// window_descriptor_ok), built with -fsanitize=address,undefined and run on the CPU by tests/test_windows_cpu.py BEFORE the
// kernel that inlines them ever runs on a GPU: they are the kernel's bounds logic.
//   windows_host <geometry.bin>
// 1. The integer geometry equals center_crop_geometry for every h, w in 1 .. 300 and for the sides {1, 2, 255, 256, 257, 32767,
//    65535} crossed, with (resize, crop) in {(256, 224), (36, 32), (36, 33), (8, 8)}; every record (h, w, resize, crop, nh, nw,
//    top, left as int32) goes to <geometry.bin>, where the Python test compares it with transform.resized_hw / crop_offsets.
// 2. window_descriptor_ok's verdicts: the edge words by hand, then random words against a 128-bit restatement of the rule.
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <random>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

using tsm_host::CropGeometry;

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

static const int kPairs[4][2] = {{256, 224}, {36, 32}, {36, 33}, {8, 8}};

static void geometry_case(int h, int w, int resize, int crop, std::FILE *out) {
  CropGeometry a{-1, -1, -1, -1}, b{-2, -2, -2, -2};
  const bool oa = tsm_host::center_crop_geometry(h, w, resize, crop, &a);
  const bool ob = tsm_host::center_crop_geometry_int(h, w, resize, crop, &b);
  EXPECT(oa == ob, "%d x %d resize %d crop %d: %d vs %d", h, w, resize, crop, (int)oa, (int)ob);
  if (oa && ob)
    EXPECT(a.nh == b.nh && a.nw == b.nw && a.top == b.top && a.left == b.left, "%d x %d resize %d crop %d: (%d %d %d %d) vs (%d %d %d %d)", h,
           w, resize, crop, a.nh, a.nw, a.top, a.left, b.nh, b.nw, b.top, b.left);
  if (out && ob) {
    const int32_t rec[8] = {h, w, resize, crop, b.nh, b.nw, b.top, b.left};
    std::fwrite(rec, sizeof rec, 1, out);
  }
}

static void geometry(std::FILE *out) {
  const int sides[7] = {1, 2, 255, 256, 257, 32767, 65535};
  for (const auto &rc : kPairs) {
    for (int h = 1; h <= 300; ++h)
      for (int w = 1; w <= 300; ++w) geometry_case(h, w, rc[0], rc[1], out);
    for (int h : sides)
      for (int w : sides) geometry_case(h, w, rc[0], rc[1], out);
  }
  // a crop larger than the resized frame is refused by both (the short side is `resize`)
  for (int h : {1, 40, 56, 300})
    for (int w : {1, 40, 56, 300}) geometry_case(h, w, 32, 36, nullptr);
  CropGeometry g;
  EXPECT(!tsm_host::center_crop_geometry_int(40, 56, 32, 36, &g), "crop 36 of a frame resized to 32");
  // the long side leaves int32: refused, not truncated
  EXPECT(!tsm_host::center_crop_geometry_int(65535, 1, INT32_MAX, 1, &g), "long side of 2^31 * 65535");
  EXPECT(!tsm_host::center_crop_geometry_int(1, 65535, 1 << 20, 1, &g), "long side of 2^20 * 65535");
}

// the rule of include/tsm_hip.h restated in 128 bits
static bool want_ok(const int32_t d[8], int n_segment, int elem, int64_t arena_bytes, bool center, int resize, int crop) {
  const __int128 off = (__int128)d[1] * ((__int128)1 << 32) + (uint32_t)d[0];
  if (off < 0 || off % 16 != 0) return false;
  if (d[2] < 1 || d[2] > 65535 || d[3] < 1 || d[3] > 65535) return false;
  if (off + (__int128)n_segment * d[2] * d[3] * 3 * elem > (__int128)arena_bytes) return false;
  if (center) {
    const __int128 lng = d[2] <= d[3] ? (__int128)resize * d[3] / d[2] : (__int128)resize * d[2] / d[3];
    if (crop > resize || crop > lng || lng > INT32_MAX) return false;
  }
  return true;
}

struct Desc {
  int32_t d[8];
};
static Desc desc(int64_t off, int32_t h, int32_t w, int32_t top = 0, int32_t left = 0, int32_t bh = 0, int32_t bw = 0) {
  return Desc{{(int32_t)(uint32_t)((uint64_t)off & 0xFFFFFFFFu), (int32_t)(off >> 32), h, w, top, left, bh, bw}};
}

static bool verdict(const Desc &x, int n_segment, int elem, int64_t arena_bytes, bool center, int resize, int crop, int64_t *off = nullptr,
                    CropGeometry *g = nullptr) {
  int64_t o = -1;
  CropGeometry gg{-1, -1, -1, -1};
  const bool ok = tsm_host::window_descriptor_ok(x.d, n_segment, elem, arena_bytes, center, resize, crop, &o, &gg);
  const bool want = want_ok(x.d, n_segment, elem, arena_bytes, center, resize, crop);
  EXPECT(ok == want, "{%d %d %d %d %d %d %d %d} n_segment %d elem %d arena %" PRId64 " center %d: %d, the rule says %d", x.d[0], x.d[1],
         x.d[2], x.d[3], x.d[4], x.d[5], x.d[6], x.d[7], n_segment, elem, arena_bytes, (int)center, (int)ok, (int)want);
  if (off) *off = o;
  if (g) *g = gg;
  return ok;
}

static void validity() {
  const int T = 8, H = 40, W = 56;
  const int64_t arena = 1 << 20, bytes = (int64_t)T * H * W * 3;       // u8: 53760, and arena - bytes is a multiple of 16
  const int32_t edge[3] = {INT32_MIN, INT32_MAX, 0};
  int64_t off;
  // the same edge value in every word
  for (int32_t e : edge) {
    const Desc x{{e, e, e, e, e, e, e, e}};
    for (int center = 0; center < 2; ++center) EXPECT(!verdict(x, T, 1, arena, center, 36, 32), "every word %d", e);
  }
  // one edge value in one word of a valid descriptor: only off_lo = 0 / off_hi = 0 (they are 0 already) and the box words pass
  for (int word = 0; word < 8; ++word)
    for (int32_t e : edge) {
      Desc x = desc(0, H, W, 5, 7, 20, 17);
      x.d[word] = e;
      const bool want = word >= 4 || (word <= 1 && e == 0);
      for (int center = 0; center < 2; ++center)
        EXPECT(verdict(x, T, 1, arena, center, 36, 32) == want, "word %d = %d", word, e);
    }
  // offsets
  EXPECT(verdict(desc(0, H, W), T, 1, arena, false, 36, 32, &off) && off == 0, "offset 0");
  EXPECT(verdict(desc(arena - bytes, H, W), T, 1, arena, false, 36, 32, &off) && off == arena - bytes, "the last window that fits");
  EXPECT(!verdict(desc(-16, H, W), T, 1, arena, false, 36, 32), "offset -16");
  EXPECT(!verdict(desc(arena, H, W), T, 1, arena, false, 36, 32), "offset = arena_bytes");
  EXPECT(!verdict(desc(arena - bytes + 1, H, W), T, 1, arena, false, 36, 32), "one byte past the last fit");
  EXPECT(!verdict(desc(arena - bytes + 16, H, W), T, 1, arena, false, 36, 32), "one aligned step past the last fit");
  EXPECT(!verdict(desc(INT64_MAX, H, W), T, 1, arena, false, 36, 32), "offset INT64_MAX");
  EXPECT(!verdict(desc(INT64_MAX - 15, H, W), T, 1, arena, false, 36, 32), "the largest aligned offset");
  EXPECT(!verdict(desc(INT64_MAX - 15, H, W), T, 1, INT64_MAX, false, 36, 32), "... in the largest arena");
  EXPECT(!verdict(desc(INT64_MIN, H, W), T, 1, arena, false, 36, 32), "offset INT64_MIN");
  EXPECT(!verdict(desc(8, H, W), T, 1, arena, false, 36, 32), "offset 8: not a multiple of 16");
  EXPECT(!verdict(desc(4 * 16 + 4, H, W), T, 4, arena, false, 36, 32), "offset 68: not a multiple of 16");
  EXPECT(verdict(desc((int64_t)1 << 32, H, W), T, 1, ((int64_t)1 << 32) + bytes, false, 36, 32, &off) && off == (int64_t)1 << 32,
         "an offset that needs off_hi");
  EXPECT(verdict(desc(((int64_t)1 << 31) + 16, H, W), T, 1, (int64_t)1 << 33, false, 36, 32, &off) && off == ((int64_t)1 << 31) + 16,
         "an offset whose off_lo is negative as an int32");
  // float32 frames are four times the bytes
  EXPECT(verdict(desc(0, H, W), T, 4, 4 * bytes, false, 36, 32), "f32 window that fits exactly");
  EXPECT(!verdict(desc(0, H, W), T, 4, 4 * bytes - 1, false, 36, 32), "f32 window one byte short");
  EXPECT(!verdict(desc(16, H, W), T, 4, 4 * bytes, false, 36, 32), "f32 window 16 bytes late");
  // sides
  EXPECT(!verdict(desc(0, 65536, W), 1, 1, (int64_t)1 << 40, false, 36, 32), "h 65536");
  EXPECT(!verdict(desc(0, H, 65536), 1, 1, (int64_t)1 << 40, false, 36, 32), "w 65536");
  EXPECT(verdict(desc(0, 65535, 65535), T, 4, (int64_t)1 << 40, false, 36, 32), "65535 x 65535 in a 1 TiB arena");
  EXPECT(!verdict(desc(0, 65535, 65535), T, 4, (int64_t)1 << 36, false, 36, 32), "65535 x 65535 x 8 x f32 in 64 GiB");
  EXPECT(!verdict(desc(0, 65535, 65535), INT32_MAX, 4, INT64_MAX, false, 36, 32), "n_segment * frame bytes leaves int64");
  EXPECT(!verdict(desc(0, -1, W), T, 1, arena, false, 36, 32) && !verdict(desc(0, H, -1), T, 1, arena, false, 36, 32), "negative side");
  // centre-crop mode: the crop must fit the resized frame, and the geometry comes back
  CropGeometry g;
  EXPECT(verdict(desc(0, H, W), T, 1, arena, true, 36, 33, nullptr, &g) && g.nh == 36 && g.nw == 50 && g.top == 2 && g.left == 8,
         "40 x 56 -> 36 x 50, crop 33: top round(1.5) = 2, left round(8.5) = 8; got %d %d %d %d", g.nh, g.nw, g.top, g.left);
  EXPECT(!verdict(desc(0, H, W), T, 1, arena, true, 32, 36), "crop 36 of a frame resized to 32 x 44");
  EXPECT(verdict(desc(0, H, W), T, 1, arena, false, 32, 36), "... which person-crop mode does not ask");
  EXPECT(!verdict(desc(0, 65535, 1), T, 1, arena, true, INT32_MAX, 1), "resized long side leaves int32");

  // random words, the special values mixed in, against the 128-bit rule (verdict() compares)
  std::mt19937_64 rng(20240607);
  const int32_t special[] = {INT32_MIN, INT32_MAX, 0, -1, 1, 16, -16, 15, 65535, 65536, H, W, (int32_t)arena, (int32_t)(arena - bytes)};
  const int n_special = (int)(sizeof special / sizeof special[0]);
  int accepted = 0;
  for (int it = 0; it < 200000; ++it) {
    Desc x;
    for (int k = 0; k < 8; ++k) {
      const uint64_t r = rng();
      x.d[k] = (r & 3) == 0 ? (int32_t)(r >> 32) : (r & 3) == 1 ? special[(r >> 8) % n_special] : (int32_t)((r >> 8) % 400) * (k == 0 ? 16 : 1);
    }
    if ((it & 3) == 0) x.d[1] = 0;
    const uint64_t r = rng();
    const int n_segment = (r & 7) == 0 ? INT32_MAX : 1 + (int)((r >> 8) % 16);
    const int64_t ab = (r & 0x30) == 0 ? INT64_MAX : (r & 0x30) == 0x10 ? arena : 1 + (int64_t)((r >> 16) % (1 << 24));
    accepted += verdict(x, n_segment, (r & 0x40) ? 4 : 1, ab, (r & 0x80) != 0, 1 + (int)((r >> 40) % 300), 1 + (int)((r >> 50) % 300));
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
  std::printf("windows host ok\n");
  return 0;
}
