// The pure-host arithmetic of the temporal pool (csrc/tsm_host_util.h: temporal_pool_segments, temporal_pool_window,
// temporal_pool_refusal), built with -fsanitize=address,undefined and run on the CPU by tests/test_temporal_pool_cpu.py: the
// segment count behind the pool, the source frames of every output frame, and each refusal.
//   temporal_pool_host
#include <climits>
#include <cstdint>
#include <cstdio>
#include <vector>

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

// max_pool3d over time, kernel 3, stride 2, padding 1, from its definition: output t' covers 2 t' - 1 .. 2 t' + 1, the padding
// frames -1 and T left out; the output length is floor((T + 2 - 3) / 2) + 1.
static void windows() {
  using namespace tsm_host;
  for (int T = 1; T <= 64; ++T) {
    const int want = T % 2 == 0 ? T / 2 : -1;
    EXPECT(temporal_pool_segments(T) == want, "T %d: %d segments", T, temporal_pool_segments(T));
    if (want < 0) {
      const PoolWindow w = temporal_pool_window(T, 0);
      EXPECT(w.first > w.last, "odd T %d has a window", T);
      continue;
    }
    EXPECT(want == (T + 2 - 3) / 2 + 1, "T %d: the pooling formula gives %d", T, (T + 2 - 3) / 2 + 1);
    std::vector<int> reads(T, 0);
    for (int t = 0; t < want; ++t) {
      const PoolWindow w = temporal_pool_window(T, t);
      int first = INT_MAX, last = INT_MIN;
      for (int f = 2 * t - 1; f <= 2 * t + 1; ++f)
        if (f >= 0 && f < T) { first = f < first ? f : first; last = f > last ? f : last; }
      EXPECT(w.first == first && w.last == last, "T %d t' %d: [%d, %d] vs [%d, %d]", T, t, w.first, w.last, first, last);
      EXPECT(w.first >= 0 && w.last < T && w.first <= 2 * t && 2 * t <= w.last, "T %d t' %d leaves the clip", T, t);
      for (int f = w.first; f <= w.last; ++f) ++reads[f];
    }
    // the ends: the first window starts at frame 0 (no frame -1), the last one ends at T - 1; even frames feed one output,
    // odd frames two, but for the last frame of the clip
    EXPECT(temporal_pool_window(T, 0).first == 0 && temporal_pool_window(T, 0).last == 1, "T %d: first window", T);
    EXPECT(temporal_pool_window(T, want - 1).last == T - 1, "T %d: last window", T);
    for (int f = 0; f < T; ++f) EXPECT(reads[f] == (f % 2 == 0 || f == T - 1 ? 1 : 2), "T %d frame %d read by %d windows", T, f, reads[f]);
    for (int t : {-1, want, want + 1, INT_MAX, INT_MIN}) {
      const PoolWindow w = temporal_pool_window(T, t);
      EXPECT(w.first > w.last, "T %d: t' %d is no output frame", T, t);
    }
  }
  EXPECT(temporal_pool_window(2, 0).first == 0 && temporal_pool_window(2, 0).last == 1, "T = 2: max(x0, x1)");
  EXPECT(temporal_pool_segments(0) == -1 && temporal_pool_segments(-2) == -1 && temporal_pool_segments(INT_MIN) == -1, "non-positive T");
  EXPECT(temporal_pool_segments(INT_MAX) == -1 && temporal_pool_segments(INT_MAX - 1) == INT_MAX / 2, "the largest T");
  const tsm_host::PoolWindow big = temporal_pool_window(INT_MAX - 1, INT_MAX / 2 - 1);
  EXPECT(big.first == INT_MAX - 4 && big.last == INT_MAX - 2, "the largest window: [%d, %d]", big.first, big.last);
}

static void refusals() {
  using namespace tsm_host;
  EXPECT(temporal_pool_refusal(kPrecF32, 1, 8, 0) == nullptr && temporal_pool_refusal(kPrecBf16x3, 1, 8, 0) == nullptr, "f32 / bf16x3, T = 8");
  EXPECT(temporal_pool_refusal(kPrecF32, 1, 2, 0) == nullptr, "T = 2");
  EXPECT(temporal_pool_refusal(kPrecBf16, 1, 8, 0) != nullptr, "bf16");
  EXPECT(temporal_pool_refusal(kPrecF32, 0, 8, 0) != nullptr, "is_shift = 0");
  for (int T = 1; T <= 63; T += 2) EXPECT(temporal_pool_refusal(kPrecF32, 1, T, 0) != nullptr, "odd T %d", T);
  EXPECT(temporal_pool_refusal(kPrecF32, 1, 0, 0) != nullptr && temporal_pool_refusal(kPrecF32, 1, -8, 0) != nullptr, "non-positive T");
  EXPECT(temporal_pool_refusal(kPrecF32, 1, 8, 1) != nullptr, "non_local");
  // four different reasons, each naming its own
  const char *why[4] = {temporal_pool_refusal(kPrecBf16, 1, 8, 0), temporal_pool_refusal(kPrecF32, 0, 8, 0),
                        temporal_pool_refusal(kPrecF32, 1, 7, 0), temporal_pool_refusal(kPrecF32, 1, 8, 1)};
  for (int i = 0; i < 4; ++i)
    for (int j = i + 1; j < 4; ++j) EXPECT(why[i] && why[j] && std::strcmp(why[i], why[j]) != 0, "reasons %d and %d", i, j);
}

int main() {
  windows();
  refusals();
  if (failures) {
    std::printf("%d failure(s)\n", failures);
    return 1;
  }
  std::printf("temporal_pool_host ok\n");
  return 0;
}
