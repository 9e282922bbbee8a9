// ASAN + UBSAN harness for the pure-host pieces of the engine (workoutdetector_amd/csrc/tsm_host_util.h): built by
// tests/test_host_sanitizers.py with  g++ -fsanitize=address,undefined -fno-sanitize-recover=all  and run on the CPU.
// (GPU AddressSanitizer is not available on this pool; the device code is covered by the parity tests instead.)
//
//   1. fuzz loop over malformed TSM_TUNE_CACHE lines through parse_tune_line (the hand-written parser that reads
//      a user-supplied file): truncated lines, huge numbers, stray bytes, missing separators, wrong code counts.
//   2. fold_and_pack / fold_and_pack_stem_pairs / to_split / to_bf16 on ragged sizes, with the packed-buffer
//      invariants checked (every weight lands inside [cout][kp], padding stays zero, split hi+lo == value to 2^-16).
//   3. clip_window_range against an enumeration and at the ends of int32 / int64, center_crop_geometry against a table.
//   4. conv_op_check, the rules of tsm_conv_op: one row per refusal (status and message verbatim), the accepted forms the GPU
//      tests use with their derived plans, and a loop over random and extreme int32 arguments on which it must be total and
//      every accepted element count below 2^31; the segmented single-source form (TSM_CONV_CODE_SEGMENTED): its refusals and plans.
//   5. layer_geometry / conv_out_size against the per-layer values of ResNet-50, ResNet-18 / 34 and wide-ResNet-50-2.
#include <climits>
#include <cstdio>
#include <random>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

using namespace tsm_host;

static int failures = 0;
#define EXPECT(cond)                                                      \
  do {                                                                    \
    if (!(cond)) {                                                        \
      std::fprintf(stderr, "FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                         \
    }                                                                     \
  } while (0)

static void fuzz_tune_lines(unsigned seed, int rounds) {
  std::mt19937 rng(seed);
  const std::string want = "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|";
  const int kNumTiles = 7;
  // a well-formed line first
  {
    std::vector<int> codes(5, -1);
    const std::string line = want + "3,259,4,1,5\n";
    EXPECT(parse_tune_line(line.c_str(), want, kNumTiles, &codes));
    EXPECT(codes[0] == 3 && codes[1] == 259 && codes[2] == 4 && codes[3] == 1 && codes[4] == 5);
  }
  // the fusion bits survive a round trip: kCodeConv23 (conv2 + conv3 as one launch) and kCodeBlock (the whole block as one
  // launch; a parser that dropped such a line would make every rank of a multi-GPU job tune for itself again)
  {
    std::vector<int> codes(5, -1);
    const std::string line = want + "2054,1030,6,3075,4102\n";       // (4102 = 6 | kCodeConv31: conv3 also runs the next block's conv1)
    EXPECT(parse_tune_line(line.c_str(), want, kNumTiles, &codes));
    EXPECT(codes[0] == (6 | kCodeBlock) && codes[1] == (6 | kCodeConv23) && codes[2] == 6 && codes[3] == (3 | kCodeConv23 | kCodeBlock) &&
           codes[4] == (6 | kCodeConv31));
    const std::string line2 = want + "515,8198,3,3,3\n";             // (515 = 3 | kCodeTailK: tail split; 8198 = 6 | kCodeFront: conv1 also runs the stride-2 conv2)
    EXPECT(parse_tune_line(line2.c_str(), want, kNumTiles, &codes));
    EXPECT(codes[0] == (3 | kCodeTailK) && codes[1] == (6 | kCodeFront));
  }
  const char *bad[] = {"", "\n", "|", "abi3", "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3",            // too few
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,3,3",        // too many
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,9",          // tile out of range
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,35",         // reserved bits set
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,16387",      // a bit above the fusion bits
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,-1",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,3,3,3,99999999999999999999999999",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3,,3,3,3",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|3 3 3 3 3",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|256|9999,abc",
                       "abi3 gfx950 T8 224x224 dtype0 shift8 fuse1|128|3,3,3,3,3"};        // another bucket
  for (const char *b : bad) {
    std::vector<int> codes(5, -7);
    EXPECT(!parse_tune_line(b, want, kNumTiles, &codes));
    for (int c : codes) EXPECT(c == -7);   // untouched on failure
  }
  // random mutations of a good line and random byte strings
  const std::string good = want + "3,259,4,1,5\n";
  for (int r = 0; r < rounds; ++r) {
    std::string line = (rng() & 1) ? good : std::string();
    const int edits = 1 + (int)(rng() % 8);
    for (int k = 0; k < edits; ++k) {
      const int op = (int)(rng() % 4);
      const size_t pos = line.empty() ? 0 : rng() % (line.size() + 1);
      if (op == 0 || line.empty()) line.insert(pos, 1, (char)(1 + rng() % 255));
      else if (op == 1) line.erase(pos < line.size() ? pos : line.size() - 1, 1 + rng() % 4);
      else if (op == 2) line[pos < line.size() ? pos : line.size() - 1] = (char)(1 + rng() % 255);
      else line.insert(pos, "0123456789,|-\n"[rng() % 14] == 0 ? "" : std::string(1 + rng() % 30, "0123456789,|-\n"[rng() % 14]));
    }
    if (line.size() > 4000) line.resize(4000);
    std::vector<int> codes(5, -7);
    const bool ok = parse_tune_line(line.c_str(), want, kNumTiles, &codes);
    for (int c : codes) EXPECT(ok ? (c >= 0 && (c & ~kCodeValid) == 0 && (c & kCodeTileMask) < kNumTiles) : c == -7);
  }
}

static void check_packing(unsigned seed) {
  std::mt19937 rng(seed);
  std::uniform_real_distribution<float> uni(-2.f, 2.f);
  const int cases[][4] = {{64, 64, 1, 64}, {64, 64, 3, 576}, {128, 256, 1, 256}, {64, 3, 7, 224}, {96, 32, 3, 320}};
  for (const auto &c : cases) {
    const int cout = c[0], cin = c[1], k = c[2], kp = c[3], cp = k == 7 ? 4 : cin;
    std::vector<float> w((size_t)cout * cin * k * k), g(cout), b(cout), m(cout), v(cout), wp, bias;
    for (float &x : w) x = uni(rng);
    for (int o = 0; o < cout; ++o) { g[o] = 1.f + 0.25f * uni(rng); b[o] = uni(rng); m[o] = uni(rng); v[o] = 0.5f + std::fabs(uni(rng)); }
    fold_and_pack(w.data(), g.data(), b.data(), m.data(), v.data(), cout, cin, k, cp, kp, &wp, &bias);
    EXPECT(wp.size() == (size_t)cout * kp && (int)bias.size() == cout);
    const float s0 = g[0] / std::sqrt(v[0] + kBnEps);
    EXPECT(wp[0] == w[0] * s0);                                  // (o=0, ky=0, kx=0, c=0)
    for (int kk = k * k * cp; kk < kp; ++kk) EXPECT(wp[kk] == 0.f);  // K padding of row 0 stays zero
    std::vector<float> split = wp, half = wp;
    to_split(&split);
    EXPECT(split.size() == wp.size());
    const uint16_t *sp = reinterpret_cast<const uint16_t *>(split.data());
    for (size_t i = 0; i + 8 <= wp.size(); i += 8)
      for (int e = 0; e < 8; ++e) {
        const float back = bf2f(sp[2 * i + e]) + bf2f(sp[2 * i + 8 + e]);
        EXPECT(std::fabs(back - wp[i + e]) <= std::ldexp(std::fabs(wp[i + e]), -15) + 1e-30f);
      }
    to_bf16(&half);
    EXPECT(half.size() == (wp.size() + 1) / 2);
    if (k == 7) {
      std::vector<float> wq, bq;
      fold_and_pack_stem_pairs(w.data(), g.data(), b.data(), m.data(), v.data(), cout, 224, &wq, &bq);
      EXPECT(wq.size() == (size_t)cout * 224);
      EXPECT(wq[0] == 0.f);                                      // (ky 0, pair 0, pixel 0) = kx -1: zero weight
      EXPECT(wq[4] == w[0] * s0);                                // (ky 0, pair 0, pixel 1, c 0) = kx 0
      for (size_t i = 3; i < wq.size(); i += 4) EXPECT(wq[i] == 0.f);   // channel 3 is padding everywhere
    }
  }
  // conv3 weights in MFMA-fragment order (fused conv2 + conv3 kernel): a permutation of the packed matrix -- every
  // weight lands exactly once, at the slot the kernel's lane / k-group arithmetic reads it from
  for (int cmid : {64, 128}) {
    std::vector<float> w3((size_t)4 * cmid * cmid), frag, fsplit;
    for (size_t i = 0; i < w3.size(); ++i) w3[i] = (float)i + 0.25f;      // distinct, exactly representable
    pack_w3_fragments(w3.data(), cmid, &frag);
    EXPECT(frag.size() == w3.size());
    std::vector<char> seen(w3.size(), 0);
    const int wgn = cmid / 32, nkk = cmid / 8;
    for (int j = 0; j < 4; ++j)
      for (int wn = 0; wn < wgn; ++wn)
        for (int kk = 0; kk < nkk; ++kk)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 4; ++e) {
              const size_t src = (size_t)(j * cmid + wn * 32 + (lane & 31)) * cmid + 8 * kk + 4 * (lane >> 5) + e;
              EXPECT(frag[((((size_t)j * wgn + wn) * nkk + kk) * 64 + lane) * 4 + e] == w3[src]);
              EXPECT(!seen[src]);
              seen[src] = 1;
            }
    for (char c : seen) EXPECT(c);
    // split-bf16 form: hi / lo halves of the 8 channels of a k16 group, identical to what to_split() stores
    for (float &x : w3) x = uni(rng);
    pack_w3_fragments_split(w3.data(), cmid, &fsplit);
    EXPECT(fsplit.size() == w3.size());
    std::vector<float> ref = w3;
    to_split(&ref);                                            // groups of 8 consecutive k of one row: [hi x8 | lo x8]
    const uint16_t *fs = reinterpret_cast<const uint16_t *>(fsplit.data()), *rs = reinterpret_cast<const uint16_t *>(ref.data());
    const int nkq = cmid / 16;
    for (int j = 0; j < 4; ++j)
      for (int wn = 0; wn < wgn; ++wn)
        for (int kq = 0; kq < nkq; ++kq)
          for (int lane = 0; lane < 64; ++lane)
            for (int e = 0; e < 8; ++e) {
              const size_t n = (size_t)j * cmid + wn * 32 + (lane & 31), k0 = 16 * kq + 8 * (lane >> 5);
              const size_t grp = (n * cmid + k0) / 8;                         // 8-element group index in to_split's layout
              const size_t base = ((((size_t)j * wgn + wn) * (2 * nkq) + 2 * kq) * 64 + lane) * 8;
              EXPECT(fs[base + e] == rs[grp * 16 + e]);
              EXPECT(fs[base + 64 * 8 + e] == rs[grp * 16 + 8 + e]);
            }
  }
  // NaN / inf survive the bf16 conversion as NaN / inf (never as a finite number)
  EXPECT(std::isnan(bf2f(f2bf(std::nanf("")))));
  EXPECT(std::isinf(bf2f(f2bf(INFINITY))));
  EXPECT(segment_len(4608, 0) > 0 && segment_len(4608, 1) == 0 && segment_len(512, 0) == 0);
  EXPECT(tile_bucket(1) == 1 && tile_bucket(5) == 8 && tile_bucket(32) == 32 && tile_bucket(33) == 64);
}

// tail_split_point: where a segmented 64x64 launch is cut into whole-K tiles and (tile, K segment) pieces.
static void check_tail_split() {
  using tsm_host::tail_split_point;
  const size_t big = (size_t)16 << 20;
  // headline shape, 256 CUs (rounds of 1 280 tiles): layer3 3x3 (M = 50 176, Cout 256: 3 136 tiles = 2.45 rounds), layer4 3x3
  // (M = 12 544, Cout 512: 1 568 = 1.225 rounds)
  EXPECT(tail_split_point(50176, 256, 4, 256, big) == 2560);
  EXPECT(tail_split_point(12544, 512, 9, 256, big) == 1280);
  // the result is a multiple of ntn, inside (0, tiles), and the scratch holds the tail's segment sums -- for every shape
  std::mt19937 rng(7);
  for (int r = 0; r < 20000; ++r) {
    const long m = 1 + (long)(rng() % 400000);
    const int cout = 64 * (1 + (int)(rng() % 32)), nseg = 1 + (int)(rng() % 12), ncu = 1 + (int)(rng() % 320);
    const size_t scratch = (size_t)(rng() % (32u << 20));
    const long from = tail_split_point(m, cout, nseg, ncu, scratch);
    const long ntn = cout / 64, tiles = (m + 63) / 64 * ntn, slots = 5L * ncu;
    if (from == 0) continue;
    EXPECT(nseg >= 2 && from > 0 && from < tiles && from % ntn == 0 && from % 1 == 0);
    EXPECT(from <= tiles / slots * slots && tiles / slots >= 1);                       // only whole rounds stay whole-K
    EXPECT((tiles - tiles / slots * slots) * 100 <= slots * 85);                      // a nearly full last round is left alone
    EXPECT((size_t)nseg * (size_t)(m - from / ntn * 64) * (size_t)cout <= scratch);   // the segment sums of the tail rows fit
  }
  EXPECT(tail_split_point(50176, 256, 4, 256, 1000) == 0);          // scratch too small
  EXPECT(tail_split_point(5488, 512, 9, 256, big) == 0);            // 688 tiles: no whole round
  EXPECT(tail_split_point(81920, 256, 4, 256, big) == 0);           // 5 120 tiles: exactly four rounds
  EXPECT(tail_split_point(50176, 256, 1, 256, big) == 0);           // one segment: nothing to split
  EXPECT(tail_split_point(50176, 96, 4, 256, big) == 0 && tail_split_point(0, 256, 4, 256, big) == 0 && tail_split_point(50176, 256, 4, 0, big) == 0);
}

// guard_layout / guard_first_bad / guard_message: the band arithmetic of the hostile-memory buffers (tsm_conv_op, TSM_POISON=1).
static void check_guard_bands() {
  EXPECT(kPoisonWord == 0x7FC07FC0u);
  EXPECT(std::isnan(bf2f((uint16_t)(kPoisonWord >> 16))) && std::isnan(bf2f((uint16_t)(kPoisonWord & 0xffffu))));
  float as_f32;
  std::memcpy(&as_f32, &kPoisonWord, 4);
  EXPECT(std::isnan(as_f32));
  EXPECT(guard_band_bytes(0) == 4096 && guard_band_bytes(64) == 4096 && guard_band_bytes(4096) == 4096);
  EXPECT(guard_band_bytes(4097) == 4608 && guard_band_bytes(4752) == 5120 && guard_band_bytes(32 * 32 * 64 * 4) == 32 * 32 * 64 * 4);
  std::mt19937 rng(11);
  for (int r = 0; r < 20000; ++r) {
    const size_t payload = (size_t)(rng() % 300000), frame = (size_t)(rng() % 70000);
    const GuardLayout g = guard_layout(payload, frame);
    EXPECT(g.lead >= 4096 && g.lead >= frame && g.lead % 512 == 0 && g.lead < frame + 512 + 4096);
    EXPECT(g.payload >= payload && g.payload < payload + 4 && g.payload % 4 == 0);
    EXPECT(g.tail >= g.lead && g.tail < g.lead + 512 && (g.lead + g.payload + g.tail) % 512 == 0 && g.total() == g.lead + g.payload + g.tail);
    // a buffer laid out so, filled, written inside the payload only: both bands clean; one stray word on either side: found
    if (r % 200 == 0) {
      std::vector<uint32_t> buf(g.total() / 4, kPoisonWord);
      for (size_t i = 0; i < g.payload / 4; ++i) buf[g.lead / 4 + i] = (uint32_t)i;
      const uint32_t *before = buf.data(), *after = buf.data() + (g.lead + g.payload) / 4;
      EXPECT(guard_first_bad(before, g.lead / 4) == -1 && guard_first_bad(after, g.tail / 4) == -1);
      const size_t hit = rng() % (g.tail / 4);
      buf[(g.lead + g.payload) / 4 + hit] = 0x3f800000u;
      EXPECT(guard_first_bad(after, g.tail / 4) == (long)hit);
      buf[g.lead / 4 - 1] = 0;
      EXPECT(guard_first_bad(before, g.lead / 4) == (long)(g.lead / 4 - 1));
    }
  }
  EXPECT(guard_first_bad(nullptr, 0) == -1);
  const GuardLayout g = guard_layout(1000 * 4, 100 * 4);
  const std::string past = guard_message("d_ys", g, true, 0, 4, 0x3f800000u);
  EXPECT(past.find("d_ys") == 0 && past.find("after the buffer, element offset 1000 (0 bytes past its end)") != std::string::npos &&
         past.find("0x3f800000") != std::string::npos);
  const std::string pre = guard_message("d_xs", g, false, g.lead / 4 - 1, 4, 0u);
  EXPECT(pre.find("before the buffer, element offset -1 (4 bytes before its start)") != std::string::npos);
  const std::string bf = guard_message("d_rs", g, true, 3, 2, 1u);       // bf16 elements: 12 bytes = 6 elements past the end
  EXPECT(bf.find("element offset 2006 (12 bytes past its end)") != std::string::npos);
  const std::string far = guard_message("buf[0]", g, false, 0, 4, 1u);   // the far end of the band before
  EXPECT(far.find("element offset -1024 (4096 bytes before its start)") != std::string::npos);
}

// clip_window_range / center_crop_geometry: the integer parts of the frame transforms' argument checks.
static void check_frame_transform_args() {
  // the window range against an enumeration of every (clip, segment) position
  for (int total = 1; total <= 20; ++total)
    for (int first_clip = 0; first_clip <= 4; ++first_clip)
      for (int n_clips = 1; n_clips <= 3; ++n_clips)
        for (int n_segment = 1; n_segment <= 3; ++n_segment)
          for (int stride = 1; stride <= 3; ++stride)
            for (int step = stride; step <= 3 * stride; step += stride)
              for (int first_frame = 0; first_frame <= 2; ++first_frame) {
                int64_t lo = INT64_MAX, hi = INT64_MIN;
                bool tail = false;
                const int n_frames = 4 + total % 5;
                for (int c = first_clip; c < first_clip + n_clips; ++c)
                  for (int k = 0; k < n_segment; ++k) {
                    const int64_t s = (int64_t)step * c + (int64_t)stride * k;
                    if (s >= total) { tail = true; continue; }
                    const int64_t j = s / stride - first_frame;
                    lo = j < lo ? j : lo;
                    hi = j > hi ? j : hi;
                  }
                WindowRange r{};
                const bool ok = clip_window_range(total, first_clip, n_clips, n_segment, step, stride, first_frame, n_frames, &r);
                if ((int64_t)step * first_clip >= total) {          // the first clip starts past the video
                  EXPECT(!ok);
                  continue;
                }
                EXPECT(ok == (r.first >= 0 && r.last < n_frames));    // (the range is filled in either way)
                // `last` is the video's last frame once the range reaches the tail: the touched maximum where the windows leave
                // no gap between them, a bound on it otherwise
                EXPECT(r.first == lo && r.tail == tail && r.last >= hi && r.last <= (total - 1) / stride - first_frame);
                if (!tail || stride * n_segment >= step) EXPECT(r.last == hi);
              }
  // near the ends of the types: every product is of two int32, every sum stays below 2^63 (UBSAN watches)
  const int i32 = INT32_MAX;
  const int64_t i64 = INT64_MAX;
  WindowRange r{};
  EXPECT(!clip_window_range(i64, i64, i32, i32, i32, 1, 0, i64, &r));                   // first_clip * step would leave int64
  EXPECT(!clip_window_range(i64, i64 / i32 + 1, 1, 1, i32, i32, 0, i64, &r));           // the first product just past the video
  EXPECT(clip_window_range(i64, i64 / i32, i32, i32, i32, i32, 0, i64, &r) && r.tail && r.last == (i64 - 1) / i32);
  EXPECT(!clip_window_range(i64, 0, i32, i32, i32, i32, i64, i64, &r) && !r.tail && r.first == -i64 &&      // before the buffer
         r.last == ((int64_t)i32 * (i32 - 1) * 2) / i32 - i64);
  EXPECT(clip_window_range(i64, 1, i32, i32, i32, 1, 0, i64, &r) && !r.tail && r.first == i32 &&
         r.last == (int64_t)i32 * i32 + (i32 - 1));
  EXPECT(clip_window_range(1, 0, i32, i32, i32, 1, 0, 1, &r) && r.tail && r.first == 0 && r.last == 0);
  // refused arguments, each alone: a non-positive size, a step that is no multiple of the stride, negative origins
  EXPECT(!clip_window_range(0, 0, 1, 1, 1, 1, 0, 9, &r) && !clip_window_range(9, -1, 1, 1, 1, 1, 0, 9, &r) &&
         !clip_window_range(9, 0, 0, 1, 1, 1, 0, 9, &r) && !clip_window_range(9, 0, 1, 0, 1, 1, 0, 9, &r) &&
         !clip_window_range(9, 0, 1, 1, 0, 1, 0, 9, &r) && !clip_window_range(9, 0, 1, 1, 1, 0, 0, 9, &r) &&
         !clip_window_range(9, 0, 1, 1, 3, 2, 0, 9, &r) && !clip_window_range(9, 0, 1, 1, 1, 1, -1, 9, &r) &&
         !clip_window_range(9, 0, 1, 1, 1, 1, 0, 0, &r) && clip_window_range(9, 0, 1, 1, 1, 1, 0, 9, &r));
  // Resize(int) + CenterCrop: (h, w, resize, crop) -> (nh, nw, top, left); (nh - crop) / 2 = 0.5, 1.5, 2.5 round to even
  const int geo[][8] = {{240, 320, 256, 224, 256, 341, 16, 58}, {320, 240, 256, 224, 341, 256, 58, 16}, {224, 224, 224, 224, 224, 224, 0, 0},
                        {40, 56, 36, 32, 36, 50, 2, 9},         {57, 33, 36, 33, 62, 36, 14, 2},        {24, 24, 17, 17, 17, 17, 0, 0},
                        {10, 10, 33, 32, 33, 33, 0, 0},         {10, 10, 35, 32, 35, 35, 2, 2},         {10, 10, 37, 32, 37, 37, 2, 2},
                        {1080, 1920, 256, 224, 256, 455, 16, 116}, {3, 2000, 256, 224, 256, 170666, 16, 85221}};
  for (const auto &q : geo) {
    CropGeometry g{};
    EXPECT(center_crop_geometry(q[0], q[1], q[2], q[3], &g));
    EXPECT(g.nh == q[4] && g.nw == q[5] && g.top == q[6] && g.left == q[7]);
  }
  CropGeometry g{};
  EXPECT(!center_crop_geometry(240, 320, 200, 224, &g) && !center_crop_geometry(320, 240, 224, 225, &g));
  EXPECT(center_crop_geometry(1, i32, 1, 1, &g) && g.nh == 1 && g.nw == i32 && g.left == (i32 - 1) / 2);
}

// ---- conv_op_check: tsm_conv_op's rules ------------------------------------------------------------------------------------
static float dummy;   // the check compares pointers with NULL and never reads through them
static tsm_conv_args conv_args(int dtype, int n, int hw, int cin, int cout, int k, int stride) {
  tsm_conv_args a{};
  a.struct_size = sizeof a;
  a.x = a.w = a.gamma = a.beta = a.mean = a.var = &dummy;
  a.y = &dummy;
  a.n = n; a.hi = a.wi = hw; a.cin = cin; a.cout = cout; a.k = k; a.stride = stride; a.dtype = dtype;
  return a;
}
static void second_source(tsm_conv_args &a, int cin2, int hw2, int stride2) {
  a.x2 = a.w2 = a.gamma2 = a.beta2 = a.mean2 = a.var2 = &dummy;
  a.cin2 = cin2; a.hi2 = a.wi2 = hw2; a.stride2 = stride2;
}
static void shift(tsm_conv_args &a, int T, int fold_div, int target) { a.shift_segments = T; a.fold_div = fold_div; a.shift_target = target; }

static void check_conv_op_refusals() {
  const char *abi = "tsm_conv_args.struct_size must be sizeof(tsm_conv_args)";
  {
    const ConvOpPlan v = conv_op_check(nullptr);
    EXPECT(v.status == TSM_ERR_INVALID_ARG && std::string(v.message) == abi);
  }
  // every row edits an accepted 1x1 (fp32, 16 frames of 4 x 4 x 64 -> 64 channels); messages as tsm_conv_op has always worded them
  struct Row { void (*edit)(tsm_conv_args &); int status; const char *message; };
  const Row rows[] = {
      {[](tsm_conv_args &a) { a.struct_size -= 4; }, TSM_ERR_INVALID_ARG, abi},
      {[](tsm_conv_args &a) { a.dtype = 3; }, TSM_ERR_UNSUPPORTED, "bad dtype"},
      {[](tsm_conv_args &a) { a.dtype = -1; }, TSM_ERR_UNSUPPORTED, "bad dtype"},
      {[](tsm_conv_args &a) { a.x = nullptr; }, TSM_ERR_INVALID_ARG, "NULL pointer"},
      {[](tsm_conv_args &a) { a.var = nullptr; }, TSM_ERR_INVALID_ARG, "NULL pointer"},
      {[](tsm_conv_args &a) { a.y = nullptr; }, TSM_ERR_INVALID_ARG, "NULL pointer"},
      {[](tsm_conv_args &a) { a.n = 0; }, TSM_ERR_INVALID_ARG, "n, hi and wi must be positive"},
      {[](tsm_conv_args &a) { a.wi = -4; }, TSM_ERR_INVALID_ARG, "n, hi and wi must be positive"},
      {[](tsm_conv_args &a) { a.k = 5; }, TSM_ERR_UNSUPPORTED, "k must be 1, 3 or 7"},
      {[](tsm_conv_args &a) { a.stride = 3; }, TSM_ERR_UNSUPPORTED, "stride must be 1 or 2"},
      {[](tsm_conv_args &a) { a.cin = 48; }, TSM_ERR_UNSUPPORTED, "cin must be 3 (k=7) or a power of two >= 32"},
      {[](tsm_conv_args &a) { a.cin = 0; }, TSM_ERR_UNSUPPORTED, "cin must be 3 (k=7) or a power of two >= 32"},
      {[](tsm_conv_args &a) { a.k = 7; a.cin = 4; }, TSM_ERR_UNSUPPORTED, "cin must be 3 (k=7) or a power of two >= 32"},
      {[](tsm_conv_args &a) { a.dtype = TSM_DTYPE_BF16; a.cin = 32; }, TSM_ERR_UNSUPPORTED, "TSM_DTYPE_BF16 needs cin % 64 == 0"},
      {[](tsm_conv_args &a) { a.cout = 96; }, TSM_ERR_UNSUPPORTED, "cout must be a multiple of 64"},
      {[](tsm_conv_args &a) { a.cout = 0; }, TSM_ERR_UNSUPPORTED, "cout must be a multiple of 64"},
      {[](tsm_conv_args &a) { a.k = 7; a.cin = 3; a.residual = &dummy; }, TSM_ERR_INVALID_ARG, "the 7x7 stem has no residual, second source or shift"},
      {[](tsm_conv_args &a) { a.k = 7; a.cin = 3; shift(a, 8, 8, 0); }, TSM_ERR_INVALID_ARG, "the 7x7 stem has no residual, second source or shift"},
      {[](tsm_conv_args &a) { a.shift_target = 2; }, TSM_ERR_INVALID_ARG, "shift_target must be 0 or 1"},
      {[](tsm_conv_args &a) { a.k = 3; shift(a, 8, 8, 1); }, TSM_ERR_INVALID_ARG, "shift_target 1 needs a residual, a second source or a 1x1 at stride 2"},
      {[](tsm_conv_args &a) { a.residual = &dummy; shift(a, 8, 8, 0); }, TSM_ERR_INVALID_ARG,
       "a shifted input with a residual: no such launch (shift_target 1 shifts the residual)"},
      {[](tsm_conv_args &a) { second_source(a, 64, 4, 1); shift(a, 8, 8, 0); }, TSM_ERR_INVALID_ARG,
       "a shifted first source with a second source: no such launch"},
      {[](tsm_conv_args &a) { a.stride = 2; shift(a, 8, 8, 0); }, TSM_ERR_INVALID_ARG, "a shifted 1x1 at stride 2 is the identity's (shift_target 1)"},
      {[](tsm_conv_args &a) { a.k = 3; second_source(a, 64, 4, 1); }, TSM_ERR_UNSUPPORTED, "a second source needs a 1x1 main conv"},
      {[](tsm_conv_args &a) { a.residual = &dummy; second_source(a, 64, 4, 1); }, TSM_ERR_INVALID_ARG, "a second source with a residual: no such launch"},
      {[](tsm_conv_args &a) { second_source(a, 64, 4, 1); a.beta2 = nullptr; }, TSM_ERR_INVALID_ARG, "NULL pointer (second source)"},
      {[](tsm_conv_args &a) { second_source(a, 96, 4, 1); }, TSM_ERR_UNSUPPORTED, "cin2 must be a power of two >= 32 (TSM_DTYPE_BF16: >= 64)"},
      {[](tsm_conv_args &a) { a.dtype = TSM_DTYPE_BF16; second_source(a, 32, 4, 1); }, TSM_ERR_UNSUPPORTED,
       "cin2 must be a power of two >= 32 (TSM_DTYPE_BF16: >= 64)"},
      {[](tsm_conv_args &a) { second_source(a, 64, 4, 0); }, TSM_ERR_UNSUPPORTED, "stride2 must be 1 or 2"},
      {[](tsm_conv_args &a) { second_source(a, 64, 9, 2); }, TSM_ERR_INVALID_ARG, "the second source's output size must equal the main conv's"},
      {[](tsm_conv_args &a) { second_source(a, 64, 0, 1); }, TSM_ERR_INVALID_ARG, "the second source's output size must equal the main conv's"},
      {[](tsm_conv_args &a) { a.residual = &dummy; shift(a, 3, 8, 1); }, TSM_ERR_INVALID_ARG, "n must be a whole number of T-frame clips"},
      {[](tsm_conv_args &a) { shift(a, 8, 32, 0); }, TSM_ERR_UNSUPPORTED, "fp32 shifts whole 4-channel groups: fold % 4 == 0"},
      {[](tsm_conv_args &a) { a.dtype = TSM_DTYPE_BF16X3; a.residual = &dummy; shift(a, 8, 16, 1); }, TSM_ERR_UNSUPPORTED,
       "the bf16 formats shift whole 8-channel groups: fold % 8 == 0"},
      {[](tsm_conv_args &a) { a.residual = &dummy; shift(a, 8, 1, 1); }, TSM_ERR_INVALID_ARG, "2 * fold exceeds the shifted tensor's channels"},
      {[](tsm_conv_args &a) { second_source(a, 64, 4, 1); shift(a, 8, 1, 1); }, TSM_ERR_INVALID_ARG, "2 * fold exceeds the shifted tensor's channels"},
      {[](tsm_conv_args &a) { a.dtype = TSM_DTYPE_BF16; a.k = 7; a.cin = 3; a.stride = 1; }, TSM_ERR_UNSUPPORTED,
       "the bf16 formats implement the 7x7 stem for stride 2 only"},
      // the one new kind: sizes that 32-bit arithmetic cannot hold (they were undefined behaviour)
      {[](tsm_conv_args &a) { a.k = 3; a.cin = 1 << 30; }, TSM_ERR_CAPACITY, "the padded K (k * k * cin, plus cin2) must fit a 32-bit int"},
      {[](tsm_conv_args &a) { a.cin = 1 << 30; second_source(a, 1 << 30, 4, 1); }, TSM_ERR_CAPACITY,
       "the padded K (k * k * cin, plus cin2) must fit a 32-bit int"},
      {[](tsm_conv_args &a) { a.n = 1 << 20; a.hi = a.wi = 64; }, TSM_ERR_CAPACITY, "n * ho * wo (output rows) must stay below 2^31"},
      {[](tsm_conv_args &a) { a.n = INT_MAX; a.hi = a.wi = INT_MAX; }, TSM_ERR_CAPACITY, "n * ho * wo (output rows) must stay below 2^31"},
      {[](tsm_conv_args &a) { a.n = 1 << 15; a.hi = a.wi = 64; }, TSM_ERR_CAPACITY,
       "the input, the output, the second source and the packed weights must each stay below 2^31 elements"},
      {[](tsm_conv_args &a) { a.cin = 1 << 16; a.cout = 1 << 16; }, TSM_ERR_CAPACITY,
       "the input, the output, the second source and the packed weights must each stay below 2^31 elements"},
      // the segmented single-source form (TSM_CONV_CODE_SEGMENTED): refused, never ignored, where no segmented kernel exists
      {[](tsm_conv_args &a) { a.cin = 1024; a.dtype = TSM_DTYPE_BF16X3; a.code = 3 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a segmented conv is fp32 only"},
      {[](tsm_conv_args &a) { a.cin = 1024; a.dtype = TSM_DTYPE_BF16; a.code = TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a segmented conv is fp32 only"},
      {[](tsm_conv_args &a) { a.k = 7; a.cin = 3; a.stride = 2; a.code = 3 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "the 7x7 stem has no segmented form"},
      {[](tsm_conv_args &a) { a.cin = 1024; a.residual = &dummy; a.code = 3 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a conv with a residual has no segmented form"},
      {[](tsm_conv_args &a) { a.k = 3; a.cin = 128; a.residual = &dummy; shift(a, 8, 8, 1); a.code = 4 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG,
       "a conv with a residual has no segmented form"},
      {[](tsm_conv_args &a) { a.cin = 1024; second_source(a, 1024, 4, 1); a.code = 3 | 0x100 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG,
       "a second source is segmented by its whole K already: the segmented bit is a single source's"},
      {[](tsm_conv_args &a) { a.k = 3; a.cin = 128; shift(a, 8, 8, 0); a.code = 3 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a shifted 3x3 has no segmented form"},
      {[](tsm_conv_args &a) { a.code = 3 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a segmented conv needs at least 32 K-steps (k * k * cin >= 1024)"},
      {[](tsm_conv_args &a) { a.cin = 512; a.code = TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG, "a segmented conv needs at least 32 K-steps (k * k * cin >= 1024)"},
      {[](tsm_conv_args &a) { a.k = 3; a.cin = 64; a.code = 3 | 0x200 | TSM_CONV_CODE_SEGMENTED; }, TSM_ERR_INVALID_ARG,
       "a segmented conv needs at least 32 K-steps (k * k * cin >= 1024)"},
  };
  for (const Row &r : rows) {
    tsm_conv_args a = conv_args(TSM_DTYPE_F32, 16, 4, 64, 64, 1, 1);
    EXPECT(conv_op_check(&a).status == TSM_OK);
    r.edit(a);
    const ConvOpPlan v = conv_op_check(&a);
    if (v.status != r.status || std::string(v.message) != r.message) {
      std::fprintf(stderr, "FAIL refusal row %d: got %d \"%s\", want %d \"%s\"\n", (int)(&r - rows), v.status, v.message, r.status, r.message);
      ++failures;
    }
  }
}

// The accepted forms of the per-op GPU tests, each plan against values worked out by hand.
static void check_conv_op_plans() {
  struct Want { int prec, stem, dual, T, fold, ho, cp, kp, pairs, kp2; long rows, x, y, x2, w; };
  auto same = [](const tsm_conv_args &a, const Want &w, int line) {
    const ConvOpPlan v = conv_op_check(&a), &p = v;
    const bool ok = v.status == TSM_OK && std::string(v.message).empty() && p.prec == w.prec && p.stem == (w.stem != 0) &&
                    p.dual == (w.dual != 0) && p.T == w.T && p.fold == w.fold && p.ho == w.ho && p.wo == w.ho && p.geo.cp == w.cp &&
                    p.geo.kp == w.kp && p.geo.stem_pairs == (w.pairs != 0) && p.kp2 == w.kp2 && p.rows == w.rows && p.x_elems == w.x &&
                    p.y_elems == w.y && p.x2_elems == w.x2 && p.w_elems == w.w;
    if (!ok) {
      std::fprintf(stderr, "FAIL plan at line %d: status %d \"%s\"\n", line, v.status, v.message);
      ++failures;
    }
  };
  tsm_conv_args a = conv_args(TSM_DTYPE_F32, 8, 32, 3, 64, 7, 2);      // the stem: 49 taps x 4 channels = 196 -> 224
  same(a, {0, 1, 0, 0, 0, 16, 4, 224, 0, 0, 2048, 65536, 131072, 0, 14336}, __LINE__);
  a.dtype = TSM_DTYPE_BF16X3;                                          // pixel pairs: 7 x 4 x 8 = 224
  same(a, {1, 1, 0, 0, 0, 16, 4, 224, 1, 0, 2048, 65536, 131072, 0, 14336}, __LINE__);
  a.dtype = TSM_DTYPE_BF16;                                            // ... rounded up to the bf16 K-step of 64
  same(a, {2, 1, 0, 0, 0, 16, 4, 256, 1, 0, 2048, 65536, 131072, 0, 16384}, __LINE__);
  a = conv_args(TSM_DTYPE_F32, 16, 4, 64, 64, 1, 1);                   // 1x1
  same(a, {0, 0, 0, 0, 0, 4, 64, 64, 0, 0, 256, 16384, 16384, 0, 4096}, __LINE__);
  shift(a, 8, 8, 0);                                                   // ... its input shifted
  same(a, {0, 0, 0, 8, 8, 4, 64, 64, 0, 0, 256, 16384, 16384, 0, 4096}, __LINE__);
  a = conv_args(TSM_DTYPE_BF16, 16, 4, 64, 128, 1, 1);                 // shifted residual: the fold is of cout
  a.residual = &dummy;
  shift(a, 8, 8, 1);
  same(a, {2, 0, 0, 8, 16, 4, 64, 64, 0, 0, 256, 16384, 32768, 0, 8192}, __LINE__);
  a = conv_args(TSM_DTYPE_F32, 8, 8, 64, 128, 3, 1);                   // 3x3 at stride 1
  same(a, {0, 0, 0, 0, 0, 8, 64, 576, 0, 0, 512, 32768, 65536, 0, 73728}, __LINE__);
  a = conv_args(TSM_DTYPE_BF16X3, 8, 9, 64, 128, 3, 2);                // 3x3 at stride 2 of 9 x 9: 5 x 5
  shift(a, 8, 8, 0);
  same(a, {1, 0, 0, 8, 8, 5, 64, 576, 0, 0, 200, 41472, 25600, 0, 73728}, __LINE__);
  a = conv_args(TSM_DTYPE_F32, 16, 4, 64, 64, 1, 1);                   // conv3 + downsample at stride 1, the second source shifted
  second_source(a, 256, 4, 1);
  shift(a, 8, 8, 1);
  same(a, {0, 0, 1, 8, 32, 4, 64, 64, 0, 256, 256, 16384, 16384, 65536, 20480}, __LINE__);
  second_source(a, 256, 7, 2);                                         // ... at stride 2: 7 x 7 -> 4 x 4
  a.shift_segments = 0;
  same(a, {0, 0, 1, 0, 0, 4, 64, 64, 0, 256, 256, 16384, 16384, 200704, 20480}, __LINE__);
  a = conv_args(TSM_DTYPE_F32, 16, 8, 64, 128, 1, 2);                  // the strided 1x1 of a BasicBlock's identity, shifted
  shift(a, 8, 8, 1);
  same(a, {0, 0, 0, 8, 8, 4, 64, 64, 0, 0, 256, 65536, 32768, 0, 8192}, __LINE__);
}

// The segmented single-source form: the plan carries layer_geometry's segment length exactly when the code asks for it, for the
// forms the engine segments (build_topology: Bottleneck conv1 = a shifted 1x1 at cin 1024 / 2048, conv2 = a 3x3 at stride 1 or 2
// at cin 128 .. 512; a no-shift BasicBlock's conv1), and 0 otherwise -- the default launch is untouched.
static void check_conv_op_segmented() {
  struct Row { int cin, k, stride, T, kseg, nseg; };
  const Row rows[] = {{1024, 1, 1, 8, 16, 2}, {2048, 1, 1, 8, 16, 4}, {1024, 1, 1, 0, 16, 2}, {128, 3, 1, 0, 18, 2}, {128, 3, 2, 0, 18, 2},
                      {256, 3, 1, 0, 18, 4}, {256, 3, 2, 0, 18, 4}, {512, 3, 1, 0, 16, 9}, {512, 3, 2, 0, 16, 9}, {4096, 1, 1, 0, 16, 8},
                      {8192, 1, 1, 3, 16, 16}};
  for (const Row &r : rows) {
    tsm_conv_args a = conv_args(TSM_DTYPE_F32, 24, 5, r.cin, 64, r.k, r.stride);
    if (r.T) shift(a, r.T, 8, 0);
    for (int code : {0, 3, 4, 3 | 0x100, 3 | 0x200, -1, INT_MIN, INT_MIN | TSM_CONV_CODE_SEGMENTED, -TSM_CONV_CODE_SEGMENTED}) {   // (a negative code is no code)
      a.code = code;
      const ConvOpPlan v = conv_op_check(&a);
      EXPECT(v.status == TSM_OK && v.kseg == 0 && v.geo.kseg == r.kseg);
    }
    for (int code : {0, 3, 4, 3 | 0x100, 4 | 0x100, 3 | 0x200, 0x7fff0000}) {
      a.code = code | TSM_CONV_CODE_SEGMENTED;
      const ConvOpPlan v = conv_op_check(&a);
      const int nk = v.geo.kp / 32;
      EXPECT(v.status == TSM_OK && v.kseg == r.kseg && v.geo.kp == r.k * r.k * r.cin && (nk + v.kseg - 1) / v.kseg == r.nseg);
    }
  }
  // the other formats keep their whole-K geometry: nothing to ask for
  for (int dtype : {TSM_DTYPE_BF16X3, TSM_DTYPE_BF16}) {
    tsm_conv_args a = conv_args(dtype, 24, 5, 1024, 64, 1, 1);
    const ConvOpPlan v = conv_op_check(&a);
    EXPECT(v.status == TSM_OK && v.kseg == 0 && v.geo.kseg == 0);
  }
}

// Random and extreme int32 arguments: the check is total (UBSAN watches), and whatever it accepts has counts that 32-bit
// arithmetic holds and that are what the arguments say, recomputed in 128 bits.
static void fuzz_conv_op_check(unsigned seed, int rounds) {
  std::mt19937 rng(seed);
  unsigned wild = 0;   // of 16: how often a field is not one of its likely values (per round: none, a few, most)
  auto pick = [&rng, &wild](std::initializer_list<int> likely) {
    const unsigned r = rng() % 16;
    if (r >= wild) return likely.begin()[rng() % likely.size()];
    if (r % 3 == 0) return (int)(1u << (rng() % 31));                                   // powers of two up to 2^30
    if (r % 3 == 1) return (int)rng();
    const int ends[] = {0, -1, INT_MAX, INT_MIN, -(1 << 30), INT_MAX - 1};
    return ends[rng() % 6];
  };
  int accepted = 0;
  for (int r = 0; r < rounds; ++r) {
    wild = r % 3 == 0 ? 0 : r % 3 == 1 ? 2 : 9;
    tsm_conv_args a = conv_args(pick({0, 1, 2}), pick({1, 8, 16, 64}), 1, pick({3, 32, 64, 256}), pick({64, 128, 512}), pick({1, 3, 7}), pick({1, 2}));
    a.hi = pick({1, 4, 7, 56});
    a.wi = pick({1, 4, 7, 56});
    if (rng() % 4 == 0) a.residual = &dummy;
    if (rng() % 4 == 0) second_source(a, pick({32, 64, 256}), 1, pick({1, 2}));
    const int h2 = (int)(2u * (unsigned)a.hi), w2 = (int)(2u * (unsigned)a.wi);   // (wrapping: the sizes may be extreme)
    a.hi2 = pick({a.hi, h2, (int)((unsigned)h2 - 1u)});
    a.wi2 = pick({a.wi, w2, (int)((unsigned)w2 - 1u)});
    shift(a, pick({0, 0, 8}), pick({0, 8, 4}), pick({0, 1}));
    a.code = pick({0, 0, 3, 3 | TSM_CONV_CODE_SEGMENTED, 0x100 | TSM_CONV_CODE_SEGMENTED});
    if (rng() % 64 == 0) a.y = nullptr;
    const ConvOpPlan v = conv_op_check(&a);
    EXPECT(v.message != nullptr && (v.status == TSM_OK) == (v.message[0] == 0));
    if (v.status != TSM_OK) continue;
    ++accepted;
    const ConvOpPlan &p = v;
    typedef __int128 i128;
    const i128 lim = (i128)1 << 31;
    EXPECT(p.ho > 0 && p.wo > 0 && p.geo.kp > 0 && p.geo.kp % 32 == 0 && p.kp2 % 32 == 0 && (i128)p.geo.kp + p.kp2 < lim);
    EXPECT(p.geo.kp >= (p.geo.stem_pairs ? 224 : a.k * a.k * p.geo.cp) && p.kp2 >= (p.dual ? a.cin2 : 0));
    EXPECT(p.rows == (i128)a.n * p.ho * p.wo && p.rows > 0 && p.rows < lim);
    EXPECT(p.x_elems == (i128)a.n * a.hi * a.wi * (p.stem ? 8 : a.cin) && p.x_elems > 0 && p.x_elems < lim);
    EXPECT(p.y_elems == (i128)p.rows * a.cout && p.y_elems > 0 && p.y_elems < lim);
    EXPECT(p.x2_elems == (p.dual ? (i128)a.n * a.hi2 * a.wi2 * a.cin2 : 0) && p.x2_elems < lim);
    EXPECT(p.w_elems == (i128)a.cout * (p.geo.kp + p.kp2) && p.w_elems < lim);
    EXPECT(p.fold >= 0 && (p.T > 0 || p.fold == 0));
    const bool asked = a.code > 0 && (a.code & TSM_CONV_CODE_SEGMENTED);
    EXPECT(p.kseg == (asked ? p.geo.kseg : 0) && (!asked || (p.kseg >= 16 && p.prec == kPrecF32 && !p.stem && !p.dual && !a.residual)));
  }
  EXPECT(accepted > rounds / 50);     // (the loop is not vacuous)
  std::printf("conv_op_check: %d of %d random argument sets accepted\n", accepted, rounds);
}

// layer_geometry and conv_out_size against the values the engine's topology has always had: a layer's K is k * k * cin as it
// stands (every width is a multiple of 64), but the stem's.
static void check_layer_geometry() {
  for (int prec : {kPrecF32, kPrecBf16x3, kPrecBf16}) {
    const LayerGeom stem = layer_geometry(3, 7, 2, prec);
    EXPECT(stem.cp == 4 && stem.kp == (prec == kPrecBf16 ? 256 : 224) && stem.kseg == 0 && stem.stem_pairs == (prec != kPrecF32));
    // {cin, k, stride} of conv1 / conv2 / conv3 / downsample, stage by stage
    const int r50[][3] = {{64, 1, 1},   {64, 3, 1},  {64, 1, 1},  {64, 1, 1},   {256, 1, 1},  {128, 3, 2}, {128, 1, 1}, {256, 1, 2},
                          {512, 1, 1},  {256, 3, 2}, {256, 1, 1}, {512, 1, 2},  {1024, 1, 1}, {512, 3, 2}, {512, 1, 1}, {1024, 1, 2},
                          {2048, 1, 1}, {512, 3, 1}};
    const int wide[][3] = {{64, 1, 1},   {128, 3, 1}, {128, 1, 1}, {256, 1, 1},   {256, 3, 2},  {256, 1, 1},  {512, 1, 1},
                           {512, 3, 2},  {512, 1, 1}, {1024, 1, 1}, {1024, 3, 2}, {1024, 1, 1}, {2048, 1, 1}, {1024, 3, 1}};
    const int r18[][3] = {{64, 3, 1}, {64, 3, 2}, {128, 3, 1}, {64, 1, 2}, {128, 3, 2}, {256, 3, 1}, {128, 1, 2}, {256, 3, 2}, {512, 3, 1}, {256, 1, 2}};
    auto table = [prec](const int (*rows)[3], size_t n) {
      for (size_t i = 0; i < n; ++i) {
        const LayerGeom g = layer_geometry(rows[i][0], rows[i][1], rows[i][2], prec);
        EXPECT(g.cp == rows[i][0] && g.kp == rows[i][1] * rows[i][1] * rows[i][0] && !g.stem_pairs && g.kseg == segment_len(g.kp, prec));
      }
    };
    table(r50, sizeof r50 / sizeof r50[0]);
    table(wide, sizeof wide / sizeof wide[0]);
    table(r18, sizeof r18 / sizeof r18[0]);
  }
  // the segmented fp32 layers by number: K-steps of 32, segments of about 16
  EXPECT(layer_geometry(512, 3, 1, kPrecF32).kp == 4608 && layer_geometry(512, 3, 1, kPrecF32).kseg == 16);
  EXPECT(layer_geometry(128, 3, 2, kPrecF32).kseg == 18 && layer_geometry(1024, 1, 1, kPrecF32).kseg == 16 && layer_geometry(512, 1, 1, kPrecF32).kseg == 0);
  EXPECT(layer_geometry(3, 7, 1, kPrecBf16).kp == 256 && !layer_geometry(3, 7, 1, kPrecBf16).stem_pairs);   // (only the stride-2 stem reads pairs)
  EXPECT(conv_out_size(224, 7, 2) == 112 && conv_out_size(112, 3, 2) == 56 && conv_out_size(56, 3, 1) == 56 && conv_out_size(56, 3, 2) == 28 &&
         conv_out_size(7, 1, 2) == 4 && conv_out_size(33, 7, 2) == 17 && conv_out_size(1, 3, 2) == 1 && conv_out_size(INT_MAX, 7, 1) == INT_MAX &&
         conv_out_size(INT_MAX, 1, 1) == INT_MAX);
  EXPECT(prec_of_dtype(TSM_DTYPE_F32) == kPrecF32 && prec_of_dtype(TSM_DTYPE_BF16X3) == kPrecBf16x3 && prec_of_dtype(TSM_DTYPE_BF16) == kPrecBf16 &&
         prec_of_dtype(3) == -1 && prec_of_dtype(-1) == -1 && prec_of_dtype(INT_MIN) == -1);
  EXPECT(packed_layout_of(kPrecF32) == TSM_LAYOUT_NTHWC4 && packed_layout_of(kPrecBf16x3) == TSM_LAYOUT_NTHWC8S && packed_layout_of(kPrecBf16) == TSM_LAYOUT_NTHWC8B);
  std::vector<float> v(64, 1.5f), s3 = v, h = v;
  to_storage(&v, kPrecF32);
  to_storage(&s3, kPrecBf16x3);
  to_storage(&h, kPrecBf16);
  EXPECT(v.size() == 64 && v[63] == 1.5f && s3.size() == 64 && h.size() == 32);
}

int main(int argc, char **argv) {
  check_conv_op_refusals();
  check_conv_op_plans();
  check_conv_op_segmented();
  check_layer_geometry();
  check_frame_transform_args();
  check_tail_split();
  check_guard_bands();
  const int rounds = argc > 1 ? std::atoi(argv[1]) : 20000;
  fuzz_tune_lines(1234, rounds);
  fuzz_conv_op_check(4321, 10 * rounds);
  check_packing(99);
  if (failures) {
    std::fprintf(stderr, "%d failures\n", failures);
    return 1;
  }
  std::printf("host sanitize ok (%d fuzz rounds)\n", rounds);
  return 0;
}
