// Live-balanced XCD runs of the position-major 3x3 launch (ConvParams::pos_balance) on the CPU, under ASAN + UBSAN:
// tsm_conv_rules.h::pos_balanced_runs and conv_route, against conv_igemm's workgroup -> tile map restated below.
// A stand-alone program (tests/test_pos_balance_cpu.py builds and runs it):
//   1. mapping: over frames 1x1 .. 9x9, 14x14, 2x5 and 6x3, both strides, ntn in {2, 4, 8}, N in {64, 128, 256}, whole-K and every
//      tail point tail_split_point returns for 8 .. 304 CUs, both walk directions -- the workgroups that do not return map
//      one-to-one onto the whole tiles, the pieces one-to-one onto (tail tile, segment), the grid is conv_route's, a run never
//      splits the n-tiles of a tile group, and with fewer tile groups than XCDs the empty runs hold nothing;
//   2. balance: every run's live work lies within one tile group (ntn tiles x 9 taps) of total / 8 -- from the construction;
//   3. the five headline launches at N = 256 frames: per-XCD live work, max / mean, for equal-count and for balanced runs.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "../workoutdetector_amd/csrc/tsm_host_util.h"

static int g_fail = 0;
#define EXPECT(cond, ...)                        \
  do {                                           \
    if (!(cond)) {                               \
      if (++g_fail <= 20) {                      \
        printf("FAIL %s:%d: ", __FILE__, __LINE__); \
        printf(__VA_ARGS__);                     \
        printf("\n");                            \
      }                                          \
    }                                            \
  } while (0)

using tsm::ConvParams;
using tsm::ConvRoute;

// A segmented fp32 3x3 layer as the engine launches it position-major: n frames of hi x wi pixels, c -> cout channels.
static ConvParams layer(int n, int hi, int wi, int c, int cout, int stride, bool balance) {
  const tsm_host::LayerGeom g = tsm_host::layer_geometry(c, 3, stride, tsm::kPrecF32);
  ConvParams p = tsm_host::conv_shape_params(g, 3, stride, cout, n, hi, wi, true, 0, 1, tsm::kPrecF32, false);
  p.tile = tsm::kTile64x64;
  p.pos_major = 1;
  p.pos_balance = balance ? 1 : 0;
  return p;
}

// What the launcher hands the kernel (launch_conv).
static ConvParams launched(ConvParams p, const ConvRoute &r) {
  p.ntm = r.ntm; p.ntn = r.ntn;
  p.pos_whole = r.pos_whole;
  for (int k = 0; k <= tsm::kXcds; ++k) p.pos_run[k] = r.pos_run[k];
  return p;
}

// conv_igemm's workgroup map for the segmented position-major arm, restated: workgroup `bid` of `grid` returns at once, or
// multiplies whole tile `tile`, or segment `seg` of tail tile `tile`.
struct Work { bool returns, in_tail; int tile, seg; };
static Work kernel_map(const ConvParams &p, int bid, int grid) {
  const bool tail_mode = p.ksplit == 2, balanced = p.pos_whole > 0;
  const int whole = balanced ? p.pos_whole : p.tail_from;
  const bool in_tail = tail_mode && bid >= whole;
  const int nwg = tail_mode ? p.tail_from : balanced ? p.ntm * p.ntn : grid;
  const int q = nwg >> 3, r = nwg & 7, xcd = bid & 7;
  int tile = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
  bool mirror = p.reverse != 0;
  if (balanced && !in_tail) {
    const int run = p.reverse ? 7 - xcd : xcd, first = p.pos_run[run], len = p.pos_run[run + 1] - first, idx = bid >> 3;
    if (idx >= len) return {true, false, -1, 0};
    tile = p.reverse ? first + len - 1 - idx : first + idx;
    mirror = false;
  }
  if (mirror) tile = nwg - 1 - tile;
  int seg = 0;
  if (in_tail) {
    const int u = bid - whole, n_tail = p.ntm * p.ntn - p.tail_from;
    seg = u / n_tail;
    tile = p.tail_from + (u - seg * n_tail);
  }
  return {false, in_tail, tile, seg};
}

// Live taps of whole tile `tile` (its position's), from the definition of the convolution.
static int tile_taps(const ConvParams &p, int tile) {
  const int pos = (tile / p.ntn) * 64 / p.N, oy = pos / p.Wo, ox = pos % p.Wo;
  int live = 0;
  for (int ky = 0; ky < 3; ++ky)
    for (int kx = 0; kx < 3; ++kx) {
      const int iy = oy * p.stride - p.pad + ky, ix = ox * p.stride - p.pad + kx;
      live += iy >= 0 && iy < p.Hi && ix >= 0 && ix < p.Wi;
    }
  return live;
}

static long g_launches = 0;

static void check_launch(ConvParams p, const char *what) {
  const ConvRoute r = tsm::conv_route(p, 3, 256);
  EXPECT(r.family == tsm::kFamIgemmSeg && r.pos_major, "%s: not a position-major route", what);
  if (r.family != tsm::kFamIgemmSeg || !r.pos_major) return;
  const int tiles = (int)r.tiles, n_seg = tsm::conv_num_segments(p);
  const int nwhole = p.ksplit == 2 ? p.tail_from : tiles, n_tail = tiles - nwhole;
  // the route: runs on tile-group boundaries, in order, covering [0, nwhole); the grid = 8 x the longest run + the pieces
  int longest = 0;
  EXPECT(r.pos_run[0] == 0 && r.pos_run[8] == nwhole, "%s: runs cover [%d, %d), not [0, %d)", what, r.pos_run[0], r.pos_run[8], nwhole);
  for (int x = 0; x < 8; ++x) {
    const int len = r.pos_run[x + 1] - r.pos_run[x];
    EXPECT(len >= 0 && r.pos_run[x] % r.ntn == 0, "%s: run %d = [%d, %d)", what, x, r.pos_run[x], r.pos_run[x + 1]);
    if (len > longest) longest = len;
  }
  EXPECT(r.pos_whole == 8 * longest && r.pos_whole >= nwhole, "%s: pos_whole %d, longest run %d", what, r.pos_whole, longest);
  EXPECT((long)r.grid == (long)r.pos_whole + (long)n_tail * (p.ksplit == 2 ? n_seg : 0), "%s: grid %u", what, r.grid);
  // balance, below: |work(XCD) - total / 8| <= ntn * 9, in eighths, in both walk directions
  const ConvParams kp = launched(p, r);
  long total = 0;
  for (int t = 0; t < nwhole; ++t) total += tile_taps(kp, t);
  int nonempty = 0;
  for (int x = 0; x < 8; ++x) nonempty += r.pos_run[x + 1] > r.pos_run[x];
  EXPECT(nonempty <= nwhole / r.ntn, "%s: %d runs hold tiles, %d tile groups", what, nonempty, nwhole / r.ntn);
  // the kernel's map, both walk directions
  for (int reverse = 0; reverse < 2; ++reverse) {
    p.reverse = reverse;
    const ConvParams k = launched(p, r);
    std::vector<char> whole_seen((size_t)nwhole, 0), piece_seen((size_t)n_tail * n_seg, 0);
    long returned = 0, work[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // live tile-taps of the whole tiles per XCD (workgroups b, b + 8, ..)
    for (unsigned bid = 0; bid < r.grid; ++bid) {
      const Work w = kernel_map(k, (int)bid, (int)r.grid);
      if (w.returns) { ++returned; continue; }
      if (!w.in_tail) {
        EXPECT(w.tile >= 0 && w.tile < nwhole && !whole_seen[(size_t)w.tile], "%s rev %d: workgroup %u -> whole tile %d", what, reverse, bid, w.tile);
        if (w.tile >= 0 && w.tile < nwhole) {
          whole_seen[(size_t)w.tile] = 1;
          work[bid & 7] += tile_taps(kp, w.tile);
        }
      } else {
        const bool ok = p.ksplit == 2 && w.tile >= nwhole && w.tile < tiles && w.seg >= 0 && w.seg < n_seg;
        const size_t at = ok ? (size_t)w.seg * n_tail + (w.tile - nwhole) : 0;
        EXPECT(ok && !piece_seen[at], "%s rev %d: workgroup %u -> piece (%d, %d)", what, reverse, bid, w.tile, w.seg);
        if (ok) piece_seen[at] = 1;
      }
    }
    for (int x = 0; x < 8; ++x)
      EXPECT(labs(8 * work[x] - total) <= 8L * r.ntn * 9, "%s rev %d: XCD %d holds %ld live tile-taps of %ld", what, reverse, x, work[x], total);
    long whole_n = 0, piece_n = 0;
    for (char c : whole_seen) whole_n += c;
    for (char c : piece_seen) piece_n += c;
    EXPECT(whole_n == nwhole && piece_n == (long)piece_seen.size() && returned == (long)r.pos_whole - nwhole,
           "%s rev %d: %ld of %d whole tiles, %ld of %zu pieces, %ld returned", what, reverse, whole_n, nwhole, piece_n, piece_seen.size(), returned);
  }
  ++g_launches;
}

static void check_shape(int hi, int wi, int stride) {
  for (int n : {64, 128, 256})
    for (int cout : {128, 256, 512}) {   // ntn 2, 4, 8
      char what[96];
      snprintf(what, sizeof what, "%dx%d s%d N %d cout %d", hi, wi, stride, n, cout);
      ConvParams p = layer(n, hi, wi, 128, cout, stride, true);
      check_launch(p, what);
      // equal-count runs where the request is off: the route is the one of before
      const ConvRoute off = tsm::conv_route(layer(n, hi, wi, 128, cout, stride, false), 3, 256);
      EXPECT(off.pos_major && off.pos_whole == 0 && (long)off.grid == off.tiles, "%s: pos_balance 0 changed the route", what);
      std::set<long> points;
      for (int n_cu = 8; n_cu <= 304; ++n_cu) {
        const long from = tsm_host::tail_split_point(p.M, p.Cout, tsm::conv_num_segments(p), n_cu, (size_t)1 << 40);
        if (from > 0) points.insert(from);
      }
      for (long from : points) {
        ConvParams t = p;
        t.ksplit = 2;
        t.tail_from = (int)from;
        t.ypart = const_cast<float *>(p.bias);   // (non-NULL; never read)
        snprintf(what, sizeof what, "%dx%d s%d N %d cout %d tail from %ld", hi, wi, stride, n, cout, from);
        check_launch(t, what);
      }
    }
}

// Per-XCD live work of a headline launch: max / mean with equal-count runs (the kernel's q / r split) and balanced.
static void headline(const char *name, int hi, int c, int cout, int stride, bool tail) {
  ConvParams p = layer(256, hi, hi, c, cout, stride, true);
  if (tail) {
    const long from = tsm_host::tail_split_point(p.M, p.Cout, tsm::conv_num_segments(p), 256, (size_t)1 << 40);
    if (from <= 0) return;
    p.ksplit = 2;
    p.tail_from = (int)from;
    p.ypart = const_cast<float *>(p.bias);
  }
  const ConvRoute r = tsm::conv_route(p, 3, 256);
  const ConvParams k = launched(p, r);
  const int nwhole = tail ? p.tail_from : (int)r.tiles, q = nwhole >> 3, rem = nwhole & 7;
  double eq_max = 0, eq_min = 1e30, bal_max = 0, bal_min = 1e30, total = 0;
  for (int x = 0; x < 8; ++x) {
    const int first = x < rem ? x * (q + 1) : rem * (q + 1) + (x - rem) * q, len = q + (x < rem);
    double eq = 0, bal = 0;
    for (int t = first; t < first + len; ++t) eq += tile_taps(k, t);
    for (int t = r.pos_run[x]; t < r.pos_run[x + 1]; ++t) bal += tile_taps(k, t);
    total += eq;
    eq_max = eq > eq_max ? eq : eq_max; eq_min = eq < eq_min ? eq : eq_min;
    bal_max = bal > bal_max ? bal : bal_max; bal_min = bal < bal_min ? bal : bal_min;
  }
  const double mean = total / 8;
  printf("xcd work %s %s equal %.3f %.3f balanced %.3f %.3f bound %.4f grid %u of %d\n", name, tail ? "tail" : "whole", eq_min / mean,
         eq_max / mean, bal_min / mean, bal_max / mean, r.ntn * 9 / mean, r.pos_whole, nwhole);   // (bound: one tile group over the mean)
}

int main() {
  for (int s = 1; s <= 9; ++s)
    for (int stride : {1, 2}) check_shape(s, s, stride);
  for (int stride : {1, 2}) {
    check_shape(14, 14, stride);
    check_shape(2, 5, stride);
    check_shape(6, 3, stride);
  }
  // one tile group: seven empty runs, their workgroups all return
  {
    const ConvParams p = layer(64, 1, 1, 128, 64, 1, true);
    const ConvRoute r = tsm::conv_route(p, 3, 256);
    int holding = 0;
    for (int x = 0; x < 8; ++x) holding += r.pos_run[x + 1] > r.pos_run[x];
    EXPECT(r.pos_whole == 8 && r.grid == 8 && r.pos_run[8] == 1 && holding == 1, "one tile: grid %u, %d runs hold a tile", r.grid, holding);
    check_launch(p, "1x1 N 64 cout 64");
  }
  for (bool tail : {false, true}) {
    headline("layer2.1-3.conv2", 28, 128, 128, 1, tail);
    headline("layer3.0.conv2", 28, 256, 256, 2, tail);
    headline("layer3.1-5.conv2", 14, 256, 256, 1, tail);
    headline("layer4.0.conv2", 14, 512, 512, 2, tail);
    headline("layer4.1-2.conv2", 7, 512, 512, 1, tail);
  }
  printf("launches checked: %ld\n", g_launches);
  if (g_fail) {
    printf("%d FAILED\n", g_fail);
    return 1;
  }
  printf("pos balance host ok\n");
  return 0;
}
