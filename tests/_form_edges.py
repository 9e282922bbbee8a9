"""Case table of the fused-form edge tests: the frames and segment counts that sit on both sides of every clause of the geometry
rules behind the bf16 engine's fused kernels (csrc/tsm_conv_rules.h), with the map of every stage and the verdict of every form
written out by hand.  Pure arithmetic (no torch, no GPU, nothing imported from the library): tests/test_form_edges_cpu.py
checks the verdicts against the header itself (tests/form_edges_host.cpp), tests/test_form_edges_gpu.py runs an engine at
every case.

    form          kernel                                     runs on             rule
    block         bneck_ws_kernel                            layer1.0-2          bneck_ws_valid:  layer1 w <= 64
    front         front_s2_kernel                            layer2.0            front_s2_valid:  layer1 h even, h >= 2, w <= 64
    conv31_l2     conv31_fused_kernel<128, 512, 128>         layer2.1-2 -> next  conv31_valid:    256 % T == 0, 256 / T >= 8
    conv31_l2l3   conv31_pc_kernel<128, 512, 256>            layer2.3 -> 3.0     conv31_valid:    128 % T == 0, 128 / T >= 8
    conv31_l3     conv31_pc_kernel<256, 1024, 256>           layer3.1-4 -> next  conv31_valid:    128 % T == 0, 128 / T >= 8
    conv23        conv3x3_ws_kernel<true>                    layer1.1-2          conv23_ws_valid: ws_tile_geometry, tile columns <= 128

The maps come from the host's conv_out_size, (n + 2 pad - k) / stride + 1, restated below and never imported: the stem is a
7 x 7 / 2 pad 3 conv, layer1's map its 3 x 3 / 2 pad 1 max-pool, layer2 and layer3 a 3 x 3 / 2 pad 1 conv further each.  The
block and conv23 forms are asked with layer1's map; so is the front (layer2.0 READS layer1's map); conv31 with layer2's or
layer3's pixel count and T.

A case is a dict: `id`, `h`, `w`, `T`, `clips`, `maps` (by hand), `tile` = the (rows, columns) of ws_tile_geometry on layer1's map
(by hand: the fewest tiles of at most 256 pixels, columns <= 128, (rows + 2) x (columns + 2) <= 352 patch pixels; ties go to the
smaller patch) and `forms`: per form (verdict, the clause that decides it, move).  `move` names the ONE constant of MOVES
which, moved by one step, flips this verdict -- the case then sits AT that clause and no other clause decides it -- or None.

`SEEDS` gives each case the seed of its input (tests/_util.make_input).  The bf16 logits bar (tests/_util.bf16_logits_report)
also asks for the oracle's arg-max, which means something only where the oracle's two largest logits of every clip lie
further apart than the two values may move, 2 x BF16_E2E_BAR of the logit scale; with seeded weights and 12 classes many
inputs are nearer ties than that (the tall frames most of all: 200 seeds gave none further apart than 0.031), so each seed is
one of 2100 + 100 k + len(id) + T at which the fp32 and the bf16-storage oracle logits both keep that distance.  The GPU test
asserts the distance before it uses the arg-max."""

FORMS = ('block', 'front', 'conv31_l2', 'conv31_l2l3', 'conv31_l3', 'conv23')
# name -> (wmax, pxmin, anyh): the arguments of tests/form_edges_host.cpp; the header's own constants are (64, 8, 0)
MOVES = {'w65': (65, 8, 0), 'w63': (63, 8, 0), 'px4': (64, 4, 0), 'px16': (64, 16, 0), 'anyh': (64, 8, 1)}
# the conv3 launch a conv31 form rides on (where conv_tiles reports its '+conv1') -> the form
CONV31_OF = {'layer2.1.conv3': 'conv31_l2', 'layer2.2.conv3': 'conv31_l2', 'layer2.3.conv3': 'conv31_l2l3',
             **{f'layer3.{b}.conv3': 'conv31_l3' for b in (1, 2, 3, 4)}}
W, HE, RT, RD, TG = 'w <= 64', 'h even', 'rows / T >= 8', 'rows % T == 0', 'tile geometry'
# the kernel each conv31 form launches -- the launch trace spells a line `<prefix>K3, C, N1> [<arguments>]` --, how often in one
# forward, and the conv1 launches it takes over
CONV31_KERNELS = {
    'conv31_l2': ('conv31_fused_kernel<', 'K3 = 128, C = 512, N1 = 128', 2, ('layer2.2.conv1', 'layer2.3.conv1')),
    'conv31_l2l3': ('conv31_pc_kernel<', 'K3 = 128, C = 512, N1 = 256', 1, ('layer3.0.conv1',)),
    'conv31_l3': ('conv31_pc_kernel<', 'K3 = 256, C = 1024, N1 = 256', 4, tuple(f'layer3.{b}.conv1' for b in (2, 3, 4, 5))),
}


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def tsm_maps(h, w):
    """{stage: (rows, columns)} of the TSM-ResNet-50 trunk on an h x w frame, down to layer3."""
    m = {'stem': (conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3))}
    prev = 'stem'
    for name in ('layer1', 'layer2', 'layer3'):
        m[name] = tuple(conv_out(v, 3, 2, 1) for v in m[prev])
        prev = name
    return m


def _conv31(l2, l2l3, l3):
    return dict(conv31_l2=l2, conv31_l2l3=l2l3, conv31_l3=l3)


_ALL31 = _conv31((True, RT, None), (True, RT, None), (True, RT, None))      # T = 4: 64 and 32 pixels per tile
_NO31 = _conv31((False, RD, None), (False, RD, None), (False, RD, None))    # T divides neither 256 nor 128
_T32 = _conv31((True, RT, 'px16'), (False, RT, 'px4'), (False, RT, 'px4'))  # 256 / 32 = 8, 128 / 32 = 4

CASES = [
    # ---- the width clause: h = 32, T = 4, 2 clips ----
    dict(id='32x256', h=32, w=256, T=4, clips=2, maps=dict(stem=(16, 128), layer1=(8, 64), layer2=(4, 32), layer3=(2, 16)),
         tile=(8, 32), forms=dict(block=(True, W, 'w63'), front=(True, W, 'w63'), conv23=(True, TG, None), **_ALL31)),
    # (stem 129: an odd frame width for the stem's pixel pairs, an odd stem width for the pool)
    dict(id='32x257', h=32, w=257, T=4, clips=2, maps=dict(stem=(16, 129), layer1=(8, 65), layer2=(4, 33), layer3=(2, 17)),
         tile=(8, 22), forms=dict(block=(False, W, 'w65'), front=(False, W, 'w65'), conv23=(True, TG, None), **_ALL31)),
    dict(id='32x264', h=32, w=264, T=4, clips=2, maps=dict(stem=(16, 132), layer1=(8, 66), layer2=(4, 33), layer3=(2, 17)),
         tile=(8, 22), forms=dict(block=(False, W, None), front=(False, W, None), conv23=(True, TG, None), **_ALL31)),
    # (layer1 130 columns: past the 128-column cap, so every row is cut into several tile columns whatever the rule prefers)
    dict(id='32x520', h=32, w=520, T=4, clips=2, maps=dict(stem=(16, 260), layer1=(8, 130), layer2=(4, 65), layer3=(2, 33)),
         tile=(8, 26), forms=dict(block=(False, W, None), front=(False, W, None), conv23=(True, TG, None), **_ALL31)),
    # the transposed frames: tall, the width clause must NOT fire (an h / w exchange shows here)
    dict(id='256x32', h=256, w=32, T=4, clips=2, maps=dict(stem=(128, 16), layer1=(64, 8), layer2=(32, 4), layer3=(16, 2)),
         tile=(32, 8), forms=dict(block=(True, W, None), front=(True, HE, None), conv23=(True, TG, None), **_ALL31)),
    # (layer1 65 rows: odd, so here the front's height clause decides, alone)
    dict(id='257x32', h=257, w=32, T=4, clips=2, maps=dict(stem=(129, 16), layer1=(65, 8), layer2=(33, 4), layer3=(17, 2)),
         tile=(25, 10), forms=dict(block=(True, W, None), front=(False, HE, 'anyh'), conv23=(True, TG, None), **_ALL31)),
    dict(id='520x32', h=520, w=32, T=4, clips=2, maps=dict(stem=(260, 16), layer1=(130, 8), layer2=(65, 4), layer3=(33, 2)),
         tile=(28, 9), forms=dict(block=(True, W, None), front=(True, HE, None), conv23=(True, TG, None), **_ALL31)),
    # ---- the front's height clause: layer1 9 rows (odd) beside 10 (even) ----
    dict(id='36x64', h=36, w=64, T=4, clips=2, maps=dict(stem=(18, 32), layer1=(9, 16), layer2=(5, 8), layer3=(3, 4)),
         tile=(9, 16), forms=dict(block=(True, W, None), front=(False, HE, 'anyh'), conv23=(True, TG, None), **_ALL31)),
    dict(id='40x64', h=40, w=64, T=4, clips=2, maps=dict(stem=(20, 32), layer1=(10, 16), layer2=(5, 8), layer3=(3, 4)),
         tile=(10, 16), forms=dict(block=(True, W, None), front=(True, HE, None), conv23=(True, TG, None), **_ALL31)),
]
# ---- the T clause: 32 x 32 frames (layer2 16 pixels, layer3 4), one clip for T >= 32, two otherwise ----
_M32 = dict(stem=(16, 16), layer1=(8, 8), layer2=(4, 4), layer3=(2, 2))
_F32 = dict(block=(True, W, None), front=(True, HE, None), conv23=(True, TG, None))
CASES += [
    # T = 1, 2: tiles of 256 / 128 (conv31_pc: 128 / 64) pixels against maps of 16 and 4; a shift with no / one neighbour frame
    dict(id='T1', h=32, w=32, T=1, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_ALL31)),
    dict(id='T2', h=32, w=32, T=2, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_ALL31)),
    dict(id='T3', h=32, w=32, T=3, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_NO31)),
    dict(id='T5', h=32, w=32, T=5, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_NO31)),
    dict(id='T6', h=32, w=32, T=6, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_NO31)),
    dict(id='T12', h=32, w=32, T=12, clips=2, maps=_M32, tile=(8, 8), forms=dict(_F32, **_NO31)),
    dict(id='T32', h=32, w=32, T=32, clips=1, maps=_M32, tile=(8, 8), forms=dict(_F32, **_T32)),
    # 256 / 64 = 4: one step short; 128 / 64 = 2: further away
    dict(id='T64', h=32, w=32, T=64, clips=1, maps=_M32, tile=(8, 8),
         forms=dict(_F32, **_conv31((False, RT, 'px4'), (False, RT, None), (False, RT, None)))),
    # T = 32 with more than one conv31 tile per clip: layer2 96 pixels = 12 tiles of 8
    dict(id='T32_64x96', h=64, w=96, T=32, clips=1, maps=dict(stem=(32, 48), layer1=(16, 24), layer2=(8, 12), layer3=(4, 6)),
         tile=(16, 12), forms=dict(_F32, **_T32)),
]


SEEDS = {'32x256': 2310, '32x257': 2110, '32x264': 2110, '32x520': 2110, '256x32': 18010, '257x32': 4110, '520x32': 11410,
         '36x64': 3809, '40x64': 2909, 'T1': 2103, 'T2': 2304, 'T3': 2105, 'T5': 3207, 'T6': 2108, 'T12': 2115, 'T32': 2135,
         'T64': 2167, 'T32_64x96': 2141}


def case(case_id):
    return next(c for c in CASES if c['id'] == case_id)


def frames_tsq():
    """The distinct (h, w, T, clips) of the table, in table order."""
    seen = []
    for c in CASES:
        k = (c['h'], c['w'], c['T'], c['clips'])
        if k not in seen:
            seen.append(k)
    return seen
