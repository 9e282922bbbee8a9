// The pure-host arithmetic of TSM_LAYOUT_TDN_POOL (csrc/tsm_host_util.h: tdn_window_frame, tdn_table_frame / tdn_table_limit,
// tdn_pool_refusal, tdn_pool_source), built with -fsanitize=address,undefined and run on the CPU by tests/test_tdn_pool_cpu.py:
// the frame numbers tdn_front_pool_kernel computes -- the kernel calls the same inline functions.
//   tdn_pool_host
#include <cinttypes>
#include <cstdint>
#include <cstdio>

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

// The rule restated in 128-bit integers, nothing shared with the function under test.
static int64_t brute(int64_t first, int64_t total, int64_t clip, int k, int j, int32_t step, int32_t stride, int64_t n, int64_t pad_frame) {
  const int64_t pad = pad_frame >= 0 && pad_frame < n ? pad_frame : -1;
  if (total <= 0 || clip < 0 || k < 0 || j < 0 || j > 4 || step <= 0 || stride <= 0) return pad;
  const __int128 centre = (__int128)step * clip + (__int128)stride * k;
  if (centre >= total) return pad;
  __int128 src = centre - 2 + j;
  if (src < 0) src = 0;
  if (src > (__int128)total - 1) src = (__int128)total - 1;
  const __int128 rel = src - first;
  return rel >= 0 && rel < n ? (int64_t)rel : pad;
}

static void window_small() {
  using namespace tsm_host;
  // exhaustive over small totals, staged ranges [first, first + n), pads, both geometries: every clip up to past the end
  long checked = 0;
  for (int64_t total = 1; total <= 27; ++total)
    for (int geo = 0; geo < 3; ++geo) {
      const int32_t step = geo == 0 ? 8 : geo == 1 ? 3 : 1, stride = geo == 0 ? 2 : geo == 1 ? 5 : 1;
      const int T = geo == 1 ? 3 : 8;
      for (int64_t first = -1; first <= total; ++first)
        for (int64_t n = 1; n <= total + 2; n += (n < 4 ? 1 : 5))
          for (int64_t pad = -1; pad <= n; pad += (n + 1 > 2 ? (n + 1) / 2 : 1))
            for (int64_t clip = 0; clip <= total / step + 1; ++clip)
              for (int k = 0; k < T; ++k)
                for (int j = 0; j < 5; ++j) {
                  const int64_t got = tdn_window_frame(first, total, clip, k, j, step, stride, n, pad);
                  const int64_t want = brute(first, total, clip, k, j, step, stride, n, pad);
                  EXPECT(got == want, "total %" PRId64 " first %" PRId64 " n %" PRId64 " pad %" PRId64 " clip %" PRId64 " k %d j %d: %" PRId64 " != %" PRId64,
                         total, first, n, pad, clip, k, j, got, want);
                  ++checked;
                }
    }
  EXPECT(checked > 500000, "only %ld cases", checked);
  // the clamps by hand: clip 0 reads frame 0 three times; the last frame is repeated; a centre on the last frame; past it the pad
  const int64_t want0[5] = {0, 0, 0, 1, 2};
  for (int j = 0; j < 5; ++j) EXPECT(tdn_window_frame(0, 45, 0, 0, j, 8, 2, 46, 45) == want0[j], "clip 0, j %d", j);
  const int64_t want_last[5] = {42, 43, 44, 44, 44};          // clip 5, k 2: centre 44 of 45
  for (int j = 0; j < 5; ++j) EXPECT(tdn_window_frame(0, 45, 5, 2, j, 8, 2, 46, 45) == want_last[j], "the last frame, j %d", j);
  for (int j = 0; j < 5; ++j) EXPECT(tdn_window_frame(0, 45, 5, 3, j, 8, 2, 46, 45) == 45, "past the end: the pad frame, j %d", j);
  for (int j = 0; j < 5; ++j) EXPECT(tdn_window_frame(0, 45, 5, 3, j, 8, 2, 45, 45) == -1, "a pad frame outside the pool: zero planes, j %d", j);
  for (int j = 0; j < 5; ++j) EXPECT(tdn_window_frame(0, 1, 0, 0, j, 8, 2, 2, 1) == 0, "one frame, j %d", j);
  EXPECT(tdn_window_frame(30, 45, 4, 0, 0, 8, 2, 16, 15) == 0 && tdn_window_frame(30, 45, 4, 0, 4, 8, 2, 16, 15) == 4, "a range in mid-video");
  EXPECT(tdn_window_frame(31, 45, 4, 0, 0, 8, 2, 16, 15) == 15, "a frame in front of the staged range takes the pad");
  EXPECT(tdn_window_frame(0, 45, 0, 0, 5, 8, 2, 46, 45) == 45 && tdn_window_frame(0, 45, 0, 0, -1, 8, 2, 46, 45) == 45, "j outside 0 .. 4");
}

static void window_ends() {
  using namespace tsm_host;
  const int64_t big = INT64_MAX, small = INT64_MIN;
  const int64_t totals[] = {1, 2, 45, (int64_t)INT32_MAX, (int64_t)INT32_MAX + 1, big - 2, big - 1, big};
  const int64_t clips[] = {0, 1, 5, (int64_t)INT32_MAX, big / 8, big / 8 + 1, big - 1, big, -1, small};
  const int64_t firsts[] = {0, 1, -1, 44, (int64_t)INT32_MIN, (int64_t)INT32_MAX, big - 4, big - 1, big, small, small + 1};
  const int32_t steps[] = {1, 8, INT32_MAX, 0, -1, INT32_MIN};
  const int ks[] = {0, 7, INT32_MAX, -1, INT32_MIN};
  const int64_t ns[] = {1, 46, big, 0, -1, small + 1};
  long checked = 0;
  for (int64_t total : totals)
    for (int64_t clip : clips)
      for (int64_t first : firsts)
        for (int32_t step : steps)
          for (int32_t stride : steps)
            for (int k : ks)
              for (int64_t n : ns)
                for (int64_t pad : {(int64_t)-1, (int64_t)0, n - 1, n, big, small})
                  for (int j = 0; j < 5; ++j) {
                    const int64_t got = tdn_window_frame(first, total, clip, k, j, step, stride, n, pad);
                    EXPECT(got == brute(first, total, clip, k, j, step, stride, n, pad), "ends: total %" PRId64 " clip %" PRId64 " first %" PRId64 " step %d stride %d k %d n %" PRId64 " j %d: %" PRId64,
                           total, clip, first, step, stride, k, n, j, got);
                    EXPECT(got == -1 || (got >= 0 && got < n), "a result outside the pool");
                    ++checked;
                  }
  EXPECT(checked > 1000000, "only %ld cases", checked);
  // zero- and negative-sized videos never index anything
  for (int64_t total : {(int64_t)0, (int64_t)-1, small})
    EXPECT(tdn_window_frame(0, total, 0, 0, 2, 8, 2, 10, 9) == 9 && tdn_window_frame(0, total, 0, 0, 2, 8, 2, 10, 10) == -1, "total %" PRId64, total);
}

static void table() {
  using namespace tsm_host;
  EXPECT(tdn_table_limit(0) == 0 && tdn_table_limit(-5) == 0 && tdn_table_limit(11) == 11u && tdn_table_limit(INT32_MAX) == (uint32_t)INT32_MAX &&
             tdn_table_limit((int64_t)INT32_MAX + 1) == 0x80000000u && tdn_table_limit(INT64_MAX) == 0x80000000u, "limits");
  const uint32_t lim = tdn_table_limit(11);
  EXPECT(tdn_table_frame(0, lim) == 0 && tdn_table_frame(10, lim) == 10, "inside");
  EXPECT(tdn_table_frame(11, lim) == -1 && tdn_table_frame(-1, lim) == -1 && tdn_table_frame(INT32_MIN, lim) == -1 && tdn_table_frame(INT32_MAX, lim) == -1, "outside");
  EXPECT(tdn_table_frame(INT32_MAX, tdn_table_limit(INT64_MAX)) == INT32_MAX && tdn_table_frame(INT32_MIN, tdn_table_limit(INT64_MAX)) == -1, "a pool beyond int32");
  EXPECT(tdn_table_frame(0, tdn_table_limit(0)) == -1, "an empty pool");
}

static void descriptor() {
  using namespace tsm_host;
  alignas(8) static float frames[4];
  static int32_t index[40];
  tsm_tdn_pool ok{};
  ok.struct_size = sizeof(tsm_tdn_pool);
  ok.mode = 0;
  ok.frames = frames;
  ok.n_frames = 11;
  ok.index = index;
  EXPECT(sizeof(tsm_tdn_pool) == 72, "the struct is %zu bytes", sizeof(tsm_tdn_pool));
  EXPECT(tdn_pool_refusal(&ok) == nullptr, "a table descriptor");
  EXPECT(tdn_pool_refusal(nullptr) != nullptr, "NULL");
  auto refused = [&](const char *what, auto change) {
    tsm_tdn_pool d = ok;
    change(d);
    const char *why = tdn_pool_refusal(&d);
    EXPECT(why != nullptr && std::strstr(why, what) != nullptr, "%s: %s", what, why ? why : "accepted");
  };
  refused("struct_size", [](tsm_tdn_pool &d) { d.struct_size = 0; });
  refused("struct_size", [](tsm_tdn_pool &d) { d.struct_size = sizeof(tsm_tdn_pool) + 8; });
  refused("mode", [](tsm_tdn_pool &d) { d.mode = 2; });
  refused("mode", [](tsm_tdn_pool &d) { d.mode = -1; });
  refused("frames is NULL", [](tsm_tdn_pool &d) { d.frames = nullptr; });
  refused("8-byte aligned", [](tsm_tdn_pool &d) { d.frames = frames + 1; });
  refused("n_frames", [](tsm_tdn_pool &d) { d.n_frames = 0; });
  refused("n_frames", [](tsm_tdn_pool &d) { d.n_frames = INT64_MIN; });
  refused("index", [](tsm_tdn_pool &d) { d.index = nullptr; });
  tsm_tdn_pool win = ok;
  win.mode = 1;
  win.index = nullptr;
  win.total_frames = 45;
  win.clip_step = 8;
  win.clip_stride = 2;
  win.pad_frame = -1;
  EXPECT(tdn_pool_refusal(&win) == nullptr, "a window descriptor");
  ok = win;
  refused("clip_step", [](tsm_tdn_pool &d) { d.clip_step = 0; });
  refused("clip_step", [](tsm_tdn_pool &d) { d.clip_stride = INT32_MIN; });
  refused("total_frames", [](tsm_tdn_pool &d) { d.total_frames = 0; });
  // the kernel's parameter: the chunk's table rows / first clip, saturated at the end of int64
  win.first_clip = 3;
  win.first_source_frame = 22;
  win.pad_frame = 10;
  TdnPoolSource s = tdn_pool_source(win, 8, 16);
  EXPECT(s.mode == 1 && s.index == nullptr && s.first_clip == 19 && s.T == 8 && s.limit == 11u && s.pad_frame == 10 && s.first_source_frame == 22 &&
             s.total_frames == 45 && s.clip_step == 8 && s.clip_stride == 2 && s.frames == frames && s.n_frames == 11, "window source");
  win.first_clip = INT64_MAX - 3;
  EXPECT(tdn_pool_source(win, 8, 8).first_clip == INT64_MAX && tdn_pool_source(win, 8, 3).first_clip == INT64_MAX, "first_clip saturates");
  ok.mode = 0;
  ok.index = index;
  s = tdn_pool_source(ok, 3, 2);
  EXPECT(s.mode == 0 && s.index == index + 2 * 3 * 5 && s.pad_frame == -1 && s.limit == 11u, "table source");
}

int main() {
  window_small();
  window_ends();
  table();
  descriptor();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("tdn_pool_host ok\n");
  return 0;
}
