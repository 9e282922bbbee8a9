"""Case table of the non-square engine tests: the frames at which tests/test_nonlocal_gpu.py, tests/test_temporal_pool_gpu.py,
tests/test_tdn_pool_gpu.py and tests/test_tdn_ring_gpu.py run an engine whose height is not its width, and the map of every stage
at each of them.  Pure arithmetic (no torch, no GPU): tests/test_geometry_cases_cpu.py checks the recorded maps against the shapes
the float64 references produce, that every stage a feature touches is non-square in both orientations, and that one h/w exchange
per feature -- invisible at 64 x 64 -- misses the project's bars at every frame of the table.

The maps come from the host's conv_out_size, (n + 2 pad - k) / stride + 1, restated below and never imported from the library:

    TSM trunk   stem conv 7 x 7 / 2 pad 3, max-pool 3 x 3 / 2 pad 1 (= layer1's map), then a 3 x 3 / 2 pad 1 conv in front of each of
                layer2, layer3, layer4; a non-local block's keys are the 2 x 2 max-pool of its stage's map (the floor drops an odd
                row or column)
    TDN         front-end tiles of 32 x 32 input pixels (8 x 8 outputs of conv1_5); conv1_5 7 x 7 / 2 pad 3 on the 2 x 2 average pool
                (H / 4), its max-pool (H / 8: diff.stem and resnext_layer1, the ring's d); the stem and its max-pool (H / 4: stem,
                fuse1, layer1, fuse2, the ring's a); layer2 H / 8, layer3 H / 16, layer4 H / 32

A case is a dict: `h`, `w`, `T`, `clips` and what its feature needs besides (`base_model`, `dtype`); `maps` is written out by
hand where the case is made and never computed.  `TOUCHED` names, per feature, the stages whose map the feature's own code
handles: those are the ones that must not be square."""

SQUARE = (64, 64)          # what the suites ran before this table: every mutant of the CPU proof is invisible here


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def tsm_maps(h, w):
    """{stage: (rows, columns)} of a TSM-ResNet trunk on an h x w frame."""
    m = {'stem': (conv_out(h, 7, 2, 3), conv_out(w, 7, 2, 3))}
    prev = 'stem'
    for name in ('layer1', 'layer2', 'layer3', 'layer4'):
        m[name] = tuple(conv_out(v, 3, 2, 1) for v in m[prev])
        prev = name
    m['keys2'] = tuple(v // 2 for v in m['layer2'])
    m['keys3'] = tuple(v // 2 for v in m['layer3'])
    return m


def tdn_maps(h, w):
    """{stage: (rows, columns)} of a TDN-ResNet50 on an h x w frame (h and w multiples of 32)."""
    assert h % 32 == 0 and w % 32 == 0
    m = {'tiles': (h // 32, w // 32)}
    m['conv1_5'] = tuple(conv_out(v // 2, 7, 2, 3) for v in (h, w))
    m['ring_d'] = tuple(conv_out(v, 3, 2, 1) for v in m['conv1_5'])
    m['ring_a'] = tuple(conv_out(conv_out(v, 7, 2, 3), 3, 2, 1) for v in (h, w))
    prev = 'ring_a'
    for name in ('layer2', 'layer3', 'layer4'):
        m[name] = tuple(conv_out(v, 3, 2, 1) for v in m[prev])
        prev = name
    return m


R50, WRN = 'resnet50', 'wide_resnet50_2'

# 48 x 80 / 80 x 48: layer3's 3 x 5 pools to 1 x 2 -- the floor drops a row in one orientation and a column in the other;
# 32 x 64: layer3's keys are 1 x 2, the smallest the block accepts, in one direction only
NON_LOCAL = [
    dict(base_model=R50, h=48, w=80, T=8, clips=2,
         maps=dict(stem=(24, 40), layer1=(12, 20), layer2=(6, 10), layer3=(3, 5), layer4=(2, 3), keys2=(3, 5), keys3=(1, 2))),
    dict(base_model=R50, h=80, w=48, T=8, clips=2,
         maps=dict(stem=(40, 24), layer1=(20, 12), layer2=(10, 6), layer3=(5, 3), layer4=(3, 2), keys2=(5, 3), keys3=(2, 1))),
    dict(base_model=R50, h=64, w=112, T=4, clips=2,
         maps=dict(stem=(32, 56), layer1=(16, 28), layer2=(8, 14), layer3=(4, 7), layer4=(2, 4), keys2=(4, 7), keys3=(2, 3))),
    dict(base_model=R50, h=32, w=64, T=3, clips=2,
         maps=dict(stem=(16, 32), layer1=(8, 16), layer2=(4, 8), layer3=(2, 4), layer4=(1, 2), keys2=(2, 4), keys3=(1, 2))),
    dict(base_model=WRN, h=80, w=48, T=8, clips=2,
         maps=dict(stem=(40, 24), layer1=(20, 12), layer2=(10, 6), layer3=(5, 3), layer4=(3, 2), keys2=(5, 3), keys3=(2, 1))),
]

# 90 x 70, T = 6: layer1 is 23 x 18 (odd and non-square) and three segments are left behind the pool, an odd count for every
# shifted block of layer2 .. layer4 (its layer4 is 3 x 3: not a stage the pool touches)
TEMPORAL_POOL = [
    dict(h=48, w=80, T=8, clips=2, dtype='f32',
         maps=dict(stem=(24, 40), layer1=(12, 20), layer2=(6, 10), layer3=(3, 5), layer4=(2, 3))),
    dict(h=80, w=48, T=4, clips=2, dtype='f32',
         maps=dict(stem=(40, 24), layer1=(20, 12), layer2=(10, 6), layer3=(5, 3), layer4=(3, 2))),
    dict(h=90, w=70, T=6, clips=2, dtype='f32',
         maps=dict(stem=(45, 35), layer1=(23, 18), layer2=(12, 9), layer3=(6, 5), layer4=(3, 3))),
    dict(h=48, w=80, T=8, clips=2, dtype='bf16x3',
         maps=dict(stem=(24, 40), layer1=(12, 20), layer2=(6, 10), layer3=(3, 5), layer4=(2, 3))),
]

# depths (1, 1, 1, 2).  64 x 96 / 96 x 64: 2 x 3 and 3 x 2 front-end tiles; 160 x 96: 5 x 3, interior tiles with a halo on every side
TDN_DEPTHS = (1, 1, 1, 2)
TDN_POOL = [
    dict(h=64, w=96, T=3, clips=3,
         maps=dict(tiles=(2, 3), conv1_5=(16, 24), ring_d=(8, 12), ring_a=(16, 24), layer2=(8, 12), layer3=(4, 6), layer4=(2, 3))),
    dict(h=96, w=64, T=3, clips=3,
         maps=dict(tiles=(3, 2), conv1_5=(24, 16), ring_d=(12, 8), ring_a=(24, 16), layer2=(12, 8), layer3=(6, 4), layer4=(3, 2))),
    dict(h=160, w=96, T=3, clips=3,
         maps=dict(tiles=(5, 3), conv1_5=(40, 24), ring_d=(20, 12), ring_a=(40, 24), layer2=(20, 12), layer3=(10, 6), layer4=(5, 3))),
]
TDN_RING = [dict(c, T=8, clips=2) for c in TDN_POOL[:2]]

FEATURES = {'non_local': NON_LOCAL, 'temporal_pool': TEMPORAL_POOL, 'tdn_pool': TDN_POOL, 'tdn_ring': TDN_RING}
# the stages whose rows and columns the feature's own launches and buffers are sized by
TOUCHED = {'non_local': ('layer2', 'layer3', 'keys2', 'keys3'), 'temporal_pool': ('layer1',),
           'tdn_pool': ('tiles', 'conv1_5', 'ring_d', 'ring_a'), 'tdn_ring': ('ring_a', 'ring_d')}


def maps_of(feature, h, w):
    """The recorded maps of the table's (h, w) frame of ``feature`` (the first case at that frame)."""
    return next(c['maps'] for c in FEATURES[feature] if (c['h'], c['w']) == (h, w))


def frames_of(feature):
    """The distinct (h, w) of a feature's cases, in table order."""
    seen = []
    for c in FEATURES[feature]:
        if (c['h'], c['w']) not in seen:
            seen.append((c['h'], c['w']))
    return seen
