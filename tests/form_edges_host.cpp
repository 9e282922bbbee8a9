// The geometry rules of the bf16 engine's fused forms (csrc/tsm_conv_rules.h: bneck_ws_valid, front_s2_valid, conv31_valid with
// conv31_rows, conv23_ws_valid, ws_tile_geometry) on the CPU, under ASAN + UBSAN.  A stand-alone program: tests/test_form_edges_cpu.py
// builds it from the header alone, feeds it the case table of tests/_form_edges.py as numbers and compares what it prints.
//
// stdin, one case per line:   frames T  l1h l1w  l2h l2w  l3h l3w      (frames = clips x T; the maps of layer1, layer2, layer3)
// argv (all optional):        wmax pxmin anyh                          (the moved constants; default 64 8 0 = the header's own)
//
// Per case it fills the arguments Forward's block_launches fills for a shifted ResNet-50 engine (shift_div 8) and prints
//   real  <block> <front> <conv31_l2> <conv31_l2l3> <conv31_l3> <conv23>  tile <tr> <tc>
//   moved <block> <front> <conv31_l2> <conv31_l2l3> <conv31_l3>
// `real` is the header's verdict.  `moved` re-evaluates one clause with a constant moved -- w <= wmax for the whole-block and
// front forms, rows / T >= pxmin for conv31, any height instead of an even one for the front (anyh = 1) -- and leaves every OTHER
// clause to the header: the rule is asked again with the moved clause's argument replaced by a value that satisfies it (the
// width capped at 64, the height rounded up to even, one segment per clip), and the moved clause is stated here.  With the
// constants unmoved, `moved` must equal `real`: the Python test asserts it, which is what ties the clauses stated here to the
// header's.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "../workoutdetector_amd/csrc/tsm_conv_rules.h"

using tsm::Conv31Params;

struct Case {
  int n, T, l1h, l1w, l2h, l2w, l3h, l3w;
};

// conv3 of a block + shift + conv1 of the next one: (K3, C, N1) and the map the block runs on; fold = the next conv1's input
// channels / shift_div
static Conv31Params conv31_params(const Case &c, int K3, int C, int N1, int hw) {
  Conv31Params q{};
  q.n_clips = c.n / c.T; q.T = c.T; q.HW = hw; q.K3 = K3; q.C = C; q.N1 = N1; q.fold = C / 8;
  return q;
}

static bool conv31_moved(const Conv31Params &q, int frames, int pxmin) {
  Conv31Params one = q;   // every other clause: one segment per clip satisfies both T clauses
  one.T = 1;
  one.n_clips = frames;
  const int rows = tsm::conv31_rows(q);
  return tsm::conv31_valid(one) && q.T > 0 && rows % q.T == 0 && rows / q.T >= pxmin;
}

int main(int argc, char **argv) {
  const int wmax = argc > 1 ? atoi(argv[1]) : 64, pxmin = argc > 2 ? atoi(argv[2]) : 8, anyh = argc > 3 ? atoi(argv[3]) : 0;
  Case c;
  int lines = 0;
  while (scanf("%d %d %d %d %d %d %d %d", &c.n, &c.T, &c.l1h, &c.l1w, &c.l2h, &c.l2w, &c.l3h, &c.l3w) == 8) {
    if (c.n <= 0 || c.T <= 0 || c.n % c.T != 0) {
      printf("FAIL bad case line %d\n", lines);
      return 1;
    }
    // the whole block: layer1.0 (cin 64) and layer1.1-2 (cin 256) on layer1's map, fold = cin / 8
    bool block = true, block_m = true;
    for (int cin : {64, 256}) {
      block = block && tsm::bneck_ws_valid(cin, c.n, c.l1h, c.l1w, c.T, cin / 8);
      block_m = block_m && tsm::bneck_ws_valid(cin, c.n, c.l1h, c.l1w < 64 ? c.l1w : 64, c.T, cin / 8) && c.l1w >= 1 && c.l1w <= wmax;
    }
    // the front: layer2.0 reads layer1's map, fold = 256 / 8
    const bool front = tsm::front_s2_valid(c.n, c.l1h, c.l1w, c.T, 32);
    const bool front_m = tsm::front_s2_valid(c.n, c.l1h + (c.l1h & 1), c.l1w < 64 ? c.l1w : 64, c.T, 32) && c.l1h >= 2 &&
                         (anyh || (c.l1h & 1) == 0) && c.l1w >= 2 && c.l1w <= wmax;
    const Conv31Params q[3] = {conv31_params(c, 128, 512, 128, c.l2h * c.l2w),     // layer2.k -> layer2.k+1
                               conv31_params(c, 128, 512, 256, c.l2h * c.l2w),     // layer2.3 -> layer3.0
                               conv31_params(c, 256, 1024, 256, c.l3h * c.l3w)};   // layer3.k -> layer3.k+1
    int tr = 0, tc = 0, tr2 = 0, tc2 = 0;
    const bool conv23 = tsm::conv23_ws_valid(c.n, c.l1h, c.l1w, &tr, &tc);
    if (tsm::ws_tile_geometry(c.l1h, c.l1w, &tr2, &tc2) != conv23 || tr2 != tr || tc2 != tc) printf("FAIL line %d: conv23_ws_valid's tile is not ws_tile_geometry's\n", lines);
    printf("real %d %d %d %d %d %d tile %d %d\n", block, front, tsm::conv31_valid(q[0]), tsm::conv31_valid(q[1]), tsm::conv31_valid(q[2]),
           conv23, tr, tc);
    printf("moved %d %d %d %d %d\n", block_m, front_m, conv31_moved(q[0], c.n, pxmin), conv31_moved(q[1], c.n, pxmin),
           conv31_moved(q[2], c.n, pxmin));
    ++lines;
  }
  printf("form edges host ok %d\n", lines);
  return 0;
}
