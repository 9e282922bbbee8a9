// The pure-host rules of the TDN forward in two phases (csrc/tsm_host_util.h: tdn_segments_refusal, tdn_ring_refusal,
// tdn_ring_slot, tdn_segments_pool, tdn_stage_in_segment_phase and the tile-cache keys), built with -fsanitize=address,undefined
// and run on the CPU by tests/test_tdn_ring_cpu.py: tdn_fuse_ring_kernel calls the same tdn_ring_slot.
//   tdn_ring_host
#include <cinttypes>
#include <climits>
#include <cstdint>
#include <cstdio>
#include <cstring>

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

static bool says(const char *why, const char *part) { return why && std::strstr(why, part); }

alignas(16) static float buf_a[8], buf_d[8], frames[8];
alignas(16) static int32_t table[8];

static tsm_tdn_segments good_segments(int mode) {
  tsm_tdn_segments d{};
  d.struct_size = sizeof(tsm_tdn_segments);
  d.mode = mode;
  d.frames = frames;
  d.n_frames = 3;
  d.index = mode == 0 ? table : nullptr;
  d.total_frames = 45;
  d.clip_step = 2;
  d.clip_stride = 2;
  d.pad_frame = 2;
  d.out_a = buf_a;
  d.out_d = buf_d;
  return d;
}

static void segments_refusals() {
  using namespace tsm_host;
  tsm_tdn_segments d = good_segments(0);
  EXPECT(tdn_segments_refusal(&d) == nullptr, "table mode: %s", tdn_segments_refusal(&d));
  d = good_segments(1);
  EXPECT(tdn_segments_refusal(&d) == nullptr, "window mode: %s", tdn_segments_refusal(&d));
  EXPECT(says(tdn_segments_refusal(nullptr), "NULL"), "null descriptor");
  d = good_segments(0);
  d.struct_size = sizeof(tsm_tdn_pool);       // the other descriptor's size: not this struct
  EXPECT(says(tdn_segments_refusal(&d), "struct_size"), "struct_size");
  d = good_segments(0); d.struct_size = 0;
  EXPECT(says(tdn_segments_refusal(&d), "struct_size"), "struct_size 0");
  d = good_segments(0); d.mode = 2;
  EXPECT(says(tdn_segments_refusal(&d), "mode"), "mode 2");
  d = good_segments(0); d.mode = -1;
  EXPECT(says(tdn_segments_refusal(&d), "mode"), "mode -1");
  d = good_segments(0); d.frames = nullptr;
  EXPECT(says(tdn_segments_refusal(&d), "frames is NULL"), "frames");
  d = good_segments(0); d.frames = reinterpret_cast<const float *>(reinterpret_cast<const char *>(frames) + 4);
  EXPECT(says(tdn_segments_refusal(&d), "8-byte"), "frames alignment");
  d = good_segments(0); d.n_frames = 0;
  EXPECT(says(tdn_segments_refusal(&d), "n_frames"), "n_frames");
  d = good_segments(0); d.n_frames = INT64_MIN;
  EXPECT(says(tdn_segments_refusal(&d), "n_frames"), "n_frames min");
  d = good_segments(0); d.index = nullptr;
  EXPECT(says(tdn_segments_refusal(&d), "index"), "index");
  d = good_segments(0); d.index = reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(table) + 2);
  EXPECT(says(tdn_segments_refusal(&d), "4-byte"), "index alignment");
  d = good_segments(1); d.clip_stride = 0;
  EXPECT(says(tdn_segments_refusal(&d), "clip_stride"), "clip_stride");
  d = good_segments(1); d.clip_stride = INT32_MIN;
  EXPECT(says(tdn_segments_refusal(&d), "clip_stride"), "clip_stride min");
  d = good_segments(1); d.clip_step = 0;      // not read: a segment is its own clip
  EXPECT(tdn_segments_refusal(&d) == nullptr, "clip_step is not read");
  d = good_segments(1); d.total_frames = 0;
  EXPECT(says(tdn_segments_refusal(&d), "total_frames"), "total_frames");
  d = good_segments(1); d.out_a = nullptr;
  EXPECT(says(tdn_segments_refusal(&d), "NULL"), "out_a");
  d = good_segments(1); d.out_d = nullptr;
  EXPECT(says(tdn_segments_refusal(&d), "NULL"), "out_d");
  d = good_segments(1); d.out_a = buf_a + 1;
  EXPECT(says(tdn_segments_refusal(&d), "16-byte"), "out_a alignment");
  d = good_segments(1); d.out_d = buf_d + 2;
  EXPECT(says(tdn_segments_refusal(&d), "16-byte"), "out_d alignment");
  // the frame fields as the pool descriptor the front end reads: one segment per clip, clip_step = clip_stride
  d = good_segments(1); d.clip_step = 77; d.first_clip = 5; d.first_source_frame = 3;
  const tsm_tdn_pool p = tdn_segments_pool(d);
  EXPECT(tdn_pool_refusal(&p) == nullptr, "%s", tdn_pool_refusal(&p));
  EXPECT(p.clip_step == 2 && p.clip_stride == 2 && p.first_clip == 5 && p.first_source_frame == 3 && p.pad_frame == 2 && p.frames == frames && p.n_frames == 3, "pool fields");
  // segment i of the phase is segment first_clip + i of the video: the window rule with T = 1
  for (int i = 0; i < 30; ++i)
    for (int j = 0; j < 5; ++j) {
      const TdnPoolSource src = tdn_pool_source(p, 1, i);
      const int64_t got = tdn_window_frame(src.first_source_frame, src.total_frames, src.first_clip, 0, j, src.clip_step, src.clip_stride, 100, 99);
      const int64_t centre = 2 * (5 + (int64_t)i);
      int64_t want = centre - 2 + j;
      if (want > 44) want = 44;
      want = centre >= 45 ? 99 : want - 3;
      EXPECT(got == want, "segment %d frame %d: %" PRId64 " != %" PRId64, i, j, got, want);
    }
}

static void ring_refusals() {
  using namespace tsm_host;
  tsm_tdn_ring good{};
  good.struct_size = sizeof(tsm_tdn_ring);
  good.n_slots = 1;
  good.ring_a = buf_a;
  good.ring_d = buf_d;
  good.table = table;
  EXPECT(tdn_ring_refusal(&good) == nullptr, "%s", tdn_ring_refusal(&good));
  EXPECT(says(tdn_ring_refusal(nullptr), "NULL"), "null descriptor");
  tsm_tdn_ring d = good; d.struct_size = sizeof(tsm_tdn_ring) + 8;
  EXPECT(says(tdn_ring_refusal(&d), "struct_size"), "struct_size");
  d = good; d.n_slots = 0;
  EXPECT(says(tdn_ring_refusal(&d), "n_slots"), "n_slots 0");
  d = good; d.n_slots = -1;
  EXPECT(says(tdn_ring_refusal(&d), "n_slots"), "n_slots -1");
  d = good; d.n_slots = INT32_MIN;
  EXPECT(says(tdn_ring_refusal(&d), "n_slots"), "n_slots min");
  d = good; d.n_slots = INT32_MAX;
  EXPECT(tdn_ring_refusal(&d) == nullptr, "n_slots max");
  d = good; d.ring_a = nullptr;
  EXPECT(says(tdn_ring_refusal(&d), "NULL"), "ring_a");
  d = good; d.ring_d = nullptr;
  EXPECT(says(tdn_ring_refusal(&d), "NULL"), "ring_d");
  d = good; d.ring_a = buf_a + 1;
  EXPECT(says(tdn_ring_refusal(&d), "16-byte"), "ring_a alignment");
  d = good; d.ring_d = buf_d + 3;
  EXPECT(says(tdn_ring_refusal(&d), "16-byte"), "ring_d alignment");
  d = good; d.table = nullptr;
  EXPECT(says(tdn_ring_refusal(&d), "table is NULL"), "table");
  d = good; d.table = reinterpret_cast<const int32_t *>(reinterpret_cast<const char *>(table) + 1);
  EXPECT(says(tdn_ring_refusal(&d), "4-byte"), "table alignment");
}

static void ring_slot() {
  using namespace tsm_host;
  for (int32_t n : {1, 2, 7, 133, INT32_MAX - 1, INT32_MAX}) {
    EXPECT(tdn_ring_slot(0, n) == 0, "n %d entry 0", n);
    EXPECT(tdn_ring_slot(n - 1, n) == n - 1, "n %d entry n - 1", n);
    EXPECT(tdn_ring_slot(n, n) == -1 || n == INT32_MAX, "n %d entry n", n);
    if (n < INT32_MAX) EXPECT(tdn_ring_slot(n + 1, n) == -1 || n + 1 == INT32_MAX, "n %d entry n + 1", n);
    EXPECT(tdn_ring_slot(-1, n) == -1, "n %d entry -1", n);
    EXPECT(tdn_ring_slot(INT32_MIN, n) == -1, "n %d INT32_MIN", n);
    EXPECT(tdn_ring_slot(INT32_MAX, n) == -1, "n %d INT32_MAX", n);     // (n_slots = INT32_MAX holds slots 0 .. INT32_MAX - 1)
  }
  EXPECT(tdn_ring_slot(133, 133) == -1 && tdn_ring_slot(134, 133) == -1 && tdn_ring_slot(132, 133) == 132, "around n_slots");
  // a ring nobody may have: nothing is a slot
  for (int32_t n : {0, -1, INT32_MIN})
    for (int32_t entry : {0, 1, -1, INT32_MIN, INT32_MAX}) EXPECT(tdn_ring_slot(entry, n) == -1, "n %d entry %d", n, entry);
  // exhaustive against the plain rule
  for (int32_t n = 1; n <= 40; ++n)
    for (int64_t entry = -50; entry <= 50; ++entry)
      EXPECT(tdn_ring_slot((int32_t)entry, n) == (entry >= 0 && entry < n ? entry : -1), "n %d entry %" PRId64, n, entry);
}

static void seam_and_keys() {
  using namespace tsm_host;
  for (const char *s : {"diff.conv1_5", "diff.stem", "stem", "fuse1", "resnext_layer1.0", "resnext_layer1.2.conv2", "layer1.0", "layer1.2.conv1"})
    EXPECT(tdn_stage_in_segment_phase(s), "%s", s);
  for (const char *s : {"fuse2", "layer2.0", "layer2.0.conv1", "layer3.1.mse.fwd", "layer4.0.shift", "layer4.1", "layer10.0", "nonsense", ""})
    EXPECT(!tdn_stage_in_segment_phase(s), "%s", s);
  EXPECT(!tdn_stage_in_segment_phase(nullptr), "null stage");
  // the phases' tile-cache keys lie above every whole forward's frame count (below 2^28) and apart from each other
  EXPECT(kTdnSegmentsKey == (1 << 28) && kTdnRingKey == (1 << 29), "keys");
  EXPECT(kTdnSegmentsKey + tile_bucket(1 << 20) < kTdnRingKey, "segment keys stay below ring keys");
}

int main() {
  std::printf("sizeof tsm_tdn_pool = %zu\nsizeof tsm_tdn_segments = %zu\nsizeof tsm_tdn_ring = %zu\n", sizeof(tsm_tdn_pool),
              sizeof(tsm_tdn_segments), sizeof(tsm_tdn_ring));
  segments_refusals();
  ring_refusals();
  ring_slot();
  seam_and_keys();
  if (failures) {
    std::printf("%d failures\n", failures);
    return 1;
  }
  std::printf("tdn_ring_host ok\n");
  return 0;
}
