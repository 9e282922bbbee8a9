"""Weights for the TSM-ResNet engine (R50, R18, R34, WRN-50-2) and the ConvNeXt-Base image model: seeded synthetic state dicts
and checkpoint key remapping.

No trained weights exist offline, so benches and parity tests use
a deterministic, numerically non-trivial state dict keyed exactly like the reference's
``TSM.state_dict()`` (workoutdetector/models/tsm.py:250-262; conv1 of every block -- Bottleneck or
BasicBlock -- is wrapped by TemporalShift, hence ``...conv1.net.weight``, tsm.py:134-136).

``remap_checkpoint_keys`` mirrors ``create_model``'s loader (tsm.py:451-473): the last two
entries of the checkpoint are the classifier, they become ``fc.weight/bias`` iff their row
count equals ``num_class``; every key loses its first dotted component.
"""
from __future__ import annotations

from collections import OrderedDict
from typing import Dict, Iterable, List, Mapping, Tuple

import numpy as np

R50_BLOCKS = (3, 4, 6, 3)
R50_PLANES = (64, 128, 256, 512)
EXPANSION = 4
# torchvision model -> (blocks per stage, block type); planes are R50_PLANES for all of them
BACKBONES = {'resnet18': ((2, 2, 2, 2), 'basic'), 'resnet34': ((3, 4, 6, 3), 'basic'),
             'resnet50': (R50_BLOCKS, 'bottleneck'), 'wide_resnet50_2': (R50_BLOCKS, 'bottleneck')}
# -> tsm_set_backbone: the depth alone (WRN-50-2 is a depth-50 schedule) ...
DEPTHS = {'resnet18': 18, 'resnet34': 34, 'resnet50': 50, 'wide_resnet50_2': 50}
# ... and -> tsm_set_bottleneck_width: torchvision's width_per_group, 64 unless listed.  A Bottleneck's mid width is
# planes * width / 64 (WRN-50-2: 128 / 256 / 512 / 1024); its output stays planes * 4.
WIDTHS = {'wide_resnet50_2': 128}
# create_model(shift_place=...) -> tsm_set_shift_place: 'blockres' wraps conv1 of every block in TemporalShift
# (``layerL.B.conv1.net.weight``), 'block' wraps every block whole (``layerL.B.net.conv1.weight``, ``layerL.B.net.bn1.*``, ...)
SHIFT_PLACES = {'blockres': 0, 'block': 1}
# create_model(non_local=True) -> tsm_set_non_local: the TSM code base's make_non_local wraps these (stage, block) pairs of a
# Bottleneck backbone in NL3DWrapper: the block's own tensors move under ``layerL.B.block``, the new ones are ``layerL.B.nl.*``
NL_BLOCKS = ((2, 0), (2, 2), (3, 0), (3, 2), (3, 4))
# make_state_dict(non_local=True): theta and phi are drawn with std gain / sqrt(C).  The scores' spread grows with gain^2, with
# sqrt(d) and with the mean square of the block's output, which rises from wrapped block to wrapped block; one gain for all five
# leaves the later ones one-hot.  These keep the largest probability of >= 98 % of the seeded R50's softmax rows inside
# (2 / N_k, 0.9) at 64 x 64 and 48 x 48 (N_k = 128 / 72 in layer2, 32 / 8 in layer3; tests/test_nonlocal_cpu.py asserts 90 %).
NL_GAINS = {(2, 0): 0.2, (2, 2): 0.16, (3, 0): 0.14, (3, 2): 0.11, (3, 4): 0.08}


# The image model the reference trains (train_img.py: timm.create_model('convnext_base'), timm 0.5.4) -> tsm_set_convnext.
# Widths are powers of two >= 128, so every GEMM of the network fits conv_igemm; the smaller variants' (96, 192, ...) do not.
CONVNEXT = 'convnext_base'
CONVNEXT_WIDTHS = (128, 256, 512, 1024)
CONVNEXT_DEPTHS = (3, 3, 27, 3)


def is_convnext(base_model: str) -> bool:
    """True for 'convnext_base'; NotImplementedError for every other ConvNeXt variant, whose widths are not powers of two
    (tiny / small: 96, 192, 384, 768; large: 192 ...; xlarge: 256 ... 2048, wider than the head kernels)."""
    if base_model == CONVNEXT:
        return True
    if isinstance(base_model, str) and base_model.startswith('convnext'):
        raise NotImplementedError(f'{base_model}: of the ConvNeXt family the engine implements {CONVNEXT} only (widths 128 .. 1024); the '
                                  "other variants' widths are not powers of two in 128 .. 1024, which conv_igemm needs")
    return False


def _backbone(base_model: str):
    if base_model not in BACKBONES:
        raise NotImplementedError(f'{base_model}: the engine implements {", ".join(sorted(BACKBONES))}')
    return BACKBONES[base_model]


def bottleneck_width(base_model: str = 'resnet50') -> int:
    """torchvision's ``width_per_group`` of ``base_model``: 128 for WRN-50-2, 64 for every other backbone."""
    _backbone(base_model)
    return WIDTHS.get(base_model, 64)


def feature_width(base_model: str = 'resnet50') -> int:
    """Channels of layer4's output = the classifier's input width: 2048 (Bottleneck), 512 (BasicBlock); 1024 for convnext_base."""
    if is_convnext(base_model):
        return CONVNEXT_WIDTHS[-1]
    return R50_PLANES[-1] * (EXPANSION if _backbone(base_model)[1] == 'bottleneck' else 1)


def _shift_place(shift_place: str) -> str:
    if shift_place not in SHIFT_PLACES:
        raise ValueError(f'shift_place must be one of {list(SHIFT_PLACES)}, got {shift_place!r}')
    return shift_place


def _non_local(non_local: bool, base_model: str) -> bool:
    if non_local and _backbone(base_model)[1] != 'bottleneck':
        raise NotImplementedError(f'non_local=True needs a Bottleneck backbone (resnet50, wide_resnet50_2), not {base_model}')
    return bool(non_local)


def nonlocal_specs(base_model: str = 'resnet50') -> List[Tuple[str, int, int]]:
    """(key prefix ``base_model.layerL.B.nl``, C, d = C // 2) of every non-local block, in forward order."""
    _non_local(True, base_model)
    return [(f'base_model.layer{li}.{b}.nl', R50_PLANES[li - 1] * EXPANSION, R50_PLANES[li - 1] * EXPANSION // 2) for li, b in NL_BLOCKS]


def nonlocal_keys(base_model: str = 'resnet50') -> List[str]:
    """The state-dict keys the non-local blocks add (NONLocalBlock3D: theta, phi = Sequential(conv, pool), g likewise,
    W = Sequential(conv, BatchNorm3d))."""
    keys = []
    for p, _c, _d in nonlocal_specs(base_model):
        keys += [p + t + s for t in ('.theta', '.phi.0', '.g.0', '.W.0') for s in ('.weight', '.bias')]
        keys += [p + '.W.1' + s for s in ('.weight', '.bias', '.running_mean', '.running_var')]
    return keys


STEM = ('base_model.conv1.weight', 'base_model.bn1', 64, 3, 7)


def block_specs(base_model: str = 'resnet50'):
    """The structure of TSM-``base_model``, one ``(stage, block, stride, convs)`` per block in forward order; ``convs``
    lists the block's convs in torchvision's module order as ``(role, cout, cin, k, stride, at_input)``: role is
    ``conv1|conv2|conv3|downsample``, ``at_input`` says whether the conv reads at the block's input size (else at its
    output size).  A Bottleneck of stage planes p is conv1 [m, cin], conv2 [m, m, 3, 3] (strided), conv3 [4p, m] and, in
    the first block of a stage, downsample [4p, cin], with mid width m = p * width / 64 (``WIDTHS``).  A BasicBlock is
    conv1 (3x3, shifted, strided), conv2 (3x3), then its downsample where the first block of a stage changes the size or
    the width."""
    blocks, kind = _backbone(base_model)
    width = bottleneck_width(base_model)
    cin = 64
    for li, (nb, planes) in enumerate(zip(blocks, R50_PLANES), start=1):
        mid, cout = (planes, planes) if kind == 'basic' else (planes * width // 64, planes * EXPANSION)
        for b in range(nb):
            s = 2 if (b == 0 and li > 1) else 1
            if kind == 'basic':
                convs = [('conv1', mid, cin, 3, s, True), ('conv2', cout, mid, 3, 1, False)]
                down = b == 0 and li > 1
            else:
                convs = [('conv1', mid, cin, 1, 1, True), ('conv2', mid, mid, 3, s, True), ('conv3', cout, mid, 1, 1, False)]
                down = b == 0
            if down:
                convs.append(('downsample', cout, cin, 1, s, True))
            yield li, b, s, convs
            cin = cout


def conv_specs(base_model: str = 'resnet50', shift_place: str = 'blockres',
               non_local: bool = False) -> List[Tuple[str, str, int, int, int]]:
    """(conv weight key, bn prefix, cout, cin, k) for every conv of TSM-``base_model``, in forward order (53 for R50 and
    WRN-50-2, 20 for R18, 36 for R34): the stem, then ``block_specs`` flattened.  ``shift_place='block'``: the same
    convs, every block's keys under its TemporalShift wrapper (``layerL.B.net.conv1.weight``, ``layerL.B.net.bn1``).
    ``non_local=True``: the same convs again, the keys of the ``NL_BLOCKS`` under ``layerL.B.block`` (the non-local blocks' own
    tensors are not convs with a BatchNorm of this form: ``nonlocal_specs`` / ``nonlocal_keys``)."""
    block = _shift_place(shift_place) == 'block'
    non_local = _non_local(non_local, base_model)
    specs = [STEM]
    for li, b, _stride, convs in block_specs(base_model):
        p = f'base_model.layer{li}.{b}' + ('.block' if non_local and (li, b) in NL_BLOCKS else '') + ('.net' if block else '')
        for role, cout, cin, k, _s, _at_input in convs:
            if role == 'downsample':
                specs.append((p + '.downsample.0.weight', p + '.downsample.1', cout, cin, k))
            else:
                wkey = '.conv1.net.weight' if (role == 'conv1' and not block) else f'.{role}.weight'
                specs.append((p + wkey, p + '.bn' + role[-1], cout, cin, k))
    return specs


def _convnext_depths(depths) -> Tuple[int, int, int, int]:
    d = tuple(int(v) for v in (CONVNEXT_DEPTHS if depths is None else depths))
    if len(d) != 4 or any(v < 1 or v > 64 for v in d):
        raise ValueError(f'convnext depths must be four stage depths in 1 .. 64, got {depths!r}')
    return d


def convnext_specs(depths=None) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, kind) of every tensor of timm 0.5.4's ``convnext_base`` without its classifier, in ``state_dict()`` order;
    ``depths``: blocks per stage, (3, 3, 27, 3) by default.  kind: ``conv`` (a conv / linear weight), ``bias``, ``ln_w`` / ``ln_b``
    (a LayerNorm's pair), ``gamma`` (a block's layer scale).  The classifier is ``head.fc.{weight [num_class, 1024], bias}``."""
    specs: List[Tuple[str, Tuple[int, ...], str]] = []

    def pair(key, shape, kinds=('conv', 'bias')):
        specs.append((key + '.weight', shape, kinds[0]))
        specs.append((key + '.bias', (shape[0],), kinds[1]))

    ln = ('ln_w', 'ln_b')
    pair('stem.0', (CONVNEXT_WIDTHS[0], 3, 4, 4))
    pair('stem.1', (CONVNEXT_WIDTHS[0],), ln)
    for s, (nb, c) in enumerate(zip(_convnext_depths(depths), CONVNEXT_WIDTHS)):
        p = f'stages.{s}'
        if s > 0:
            pair(p + '.downsample.0', (c // 2,), ln)
            pair(p + '.downsample.1', (c, c // 2, 2, 2))
        for b in range(nb):
            q = f'{p}.blocks.{b}'
            specs.append((q + '.gamma', (c,), 'gamma'))
            pair(q + '.conv_dw', (c, 1, 7, 7))
            pair(q + '.norm', (c,), ln)
            pair(q + '.mlp.fc1', (4 * c, c))
            pair(q + '.mlp.fc2', (c, 4 * c))
    pair('head.norm', (CONVNEXT_WIDTHS[-1],), ln)
    return specs


def _make_convnext_state_dict(seed: int, num_class: int, depths) -> 'OrderedDict[str, np.ndarray]':
    """The seeded ``convnext_base`` state dict, from a generator of its own (seeded from ``(seed, "cnx")``).  Conv / linear weights
    are normal with std 1 / sqrt(fan_in), their biases std 0.1; LayerNorm weights uniform in 0.8 .. 1.2, biases std 0.1; ``gamma``
    uniform in 0.1 .. 0.3 -- NOT timm's initial 1e-6, under which every block is the identity to fp32 and no test of a block could
    fail.  A block then adds a branch of about a seventh of the stream's size: over the 36 blocks the root mean square of the
    residual stream stays in 1.0 .. 1.3 (tests/test_convnext_cpu.py checks 0.5 .. 100 on the float64 model)."""
    rng = np.random.default_rng([seed, int.from_bytes(b'cnx', 'big')])
    sd: 'OrderedDict[str, np.ndarray]' = OrderedDict()
    for key, shape, kind in convnext_specs(depths) + [('head.fc.weight', (num_class, CONVNEXT_WIDTHS[-1]), 'fc'), ('head.fc.bias', (num_class,), 'bias')]:
        if kind == 'conv':
            a = rng.standard_normal(shape) / np.sqrt(float(np.prod(shape[1:])))
        elif kind == 'fc':
            a = rng.standard_normal(shape) * 0.05
        elif kind == 'ln_w':
            a = rng.uniform(0.8, 1.2, shape)
        elif kind == 'gamma':
            a = rng.uniform(0.1, 0.3, shape)
        else:
            a = rng.standard_normal(shape) * 0.1
        sd[key] = np.ascontiguousarray(a, dtype=np.float32)
    return sd


def remap_timm_keys(state_dict: Mapping[str, object]) -> 'OrderedDict[str, object]':
    """A timm ``convnext_base`` ``state_dict`` (``stem.0.weight``, ``stages.0.blocks.0.gamma``, ..., ``head.fc.*``) -> engine keys,
    which are timm's own.  The reference's Lightning checkpoint holds the model as ``classifier`` (train_img.py:28-43), so every
    key carries one leading component: it is stripped when every key has the same one and ``stem.0.weight`` is not already there.
    Anything that is not a ConvNeXt key raises."""
    keys = list(state_dict.keys())
    if not keys:
        raise ValueError('empty state dict')
    strip = 0
    if 'stem.0.weight' not in state_dict:
        heads = {k.split('.', 1)[0] for k in keys}
        if len(heads) != 1 or f'{next(iter(heads))}.stem.0.weight' not in state_dict:
            raise ValueError('not a timm ConvNeXt state dict: no stem.0.weight, with or without one leading component')
        strip = len(next(iter(heads))) + 1
    out: 'OrderedDict[str, object]' = OrderedDict()
    for k, v in state_dict.items():
        name = k[strip:]
        if name.split('.', 1)[0] not in ('stem', 'stages', 'head'):
            raise ValueError(f'{k}: not a key of a timm ConvNeXt')
        out[name] = v
    return out


# TDN-ResNet50 (models/tdn.py: TSN(backbone_fn=tdn_net)) -> tsm_set_tdn.  The keys are the TSN module's; include/tsm_hip.h holds the
# network's definition.
TDN = 'tdn_resnet50'
TDN_DEPTHS = R50_BLOCKS
TDN_FRAMES = 5


def _tdn_depths(depths) -> Tuple[int, int, int, int]:
    d = tuple(int(v) for v in (TDN_DEPTHS if depths is None else depths))
    if len(d) != 4 or any(v < 1 or v > 64 for v in d):
        raise ValueError(f'tdn depths must be four stage depths in 1 .. 64, got {depths!r}')
    return d


def tdn_alpha_beta(num_segments: int) -> Tuple[float, float]:
    """tdn_net's blend weights: 0.5, 0.5 at eight segments, else 0.75, 0.25 (models/tdn.py:189-192)."""
    return (0.5, 0.5) if num_segments == 8 else (0.75, 0.25)


def tdn_specs(depths=None) -> List[Tuple[str, Tuple[int, ...], str]]:
    """(key, shape, kind) of every tensor the engine reads from a TDN ``state_dict``, without the classifier
    (``new_fc.{weight [num_class, 2048], bias}``).  kind: ``conv`` (a 2-d conv weight), ``bias`` (a conv bias), ``bn_w`` / ``bn_b`` /
    ``bn_m`` / ``bn_v`` (a BatchNorm's weight, bias, running mean and variance), ``temporal`` (``shift.conv.weight`` [C, 1, 3])."""
    specs: List[Tuple[str, Tuple[int, ...], str]] = []

    def conv(key, cout, cin, k, bias=True, groups=1):
        specs.append((key + '.weight', (cout, cin // groups, k, k), 'conv'))
        if bias:
            specs.append((key + '.bias', (cout,), 'bias'))

    def bn(key, c):
        specs.extend((key + s, (c,), kind) for s, kind in (('.weight', 'bn_w'), ('.bias', 'bn_b'), ('.running_mean', 'bn_m'), ('.running_var', 'bn_v')))

    conv('base_model.conv1', 64, 3, 7)
    bn('base_model.bn1', 64)
    conv('base_model.conv1_5.0', 64, 12, 7, bias=False)
    bn('base_model.conv1_5.1', 64)
    d = _tdn_depths(depths)
    for li in range(0, 5):      # 0: resnext_layer1
        stage = max(li, 1) - 1
        planes, cout = R50_PLANES[stage], R50_PLANES[stage] * EXPANSION
        cin = 64 if stage == 0 else R50_PLANES[stage - 1] * EXPANSION
        for b in range(d[stage]):
            p = f'base_model.resnext_layer1.{b}' if li == 0 else f'base_model.layer{li}_bak.{b}'
            conv(p + '.conv1', planes, cin, 1)
            bn(p + '.bn1', planes)
            if li >= 2:
                r = planes // 16
                conv(p + '.mse.conv1', r, planes, 1, bias=False)
                bn(p + '.mse.bn1', r)
                conv(p + '.mse.conv2', r, r, 3, bias=False, groups=r)
                conv(p + '.mse.conv3', planes, r, 1, bias=False)
                bn(p + '.mse.bn3', planes)
                for sc in ('2', '4'):
                    conv(p + '.mse.conv3_smallscale' + sc, r, r, 3, bias=False)
                    bn(p + '.mse.bn3_smallscale' + sc, r)
                specs.append((p + '.shift.conv.weight', (planes, 1, 3), 'temporal'))
            conv(p + '.conv2', planes, planes, 3)
            bn(p + '.bn2', planes)
            conv(p + '.conv3', cout, planes, 1)
            bn(p + '.bn3', cout)
            if b == 0:
                conv(p + '.downsample.0', cout, cin, 1)
                bn(p + '.downsample.1', cout)
            cin = cout
    return specs


def make_tdn_state_dict(seed: int = 0, num_class: int = 12, depths=None) -> 'OrderedDict[str, np.ndarray]':
    """A seeded TDN state dict (numpy, torch layouts), drawn in sorted key order from ``np.random.default_rng(seed)``: conv weights
    N(0, sqrt(2 / (k * k * cout))) (FBResNet's init), conv biases N(0, 0.1), BatchNorm weight and variance U(0.5, 1.5), bias and mean
    N(0, 0.1), temporal weights N(0, 0.5), ``new_fc`` N(0, 0.05) / N(0, 0.1)."""
    specs = tdn_specs(depths) + [('new_fc.weight', (num_class, R50_PLANES[-1] * EXPANSION), 'fc'), ('new_fc.bias', (num_class,), 'bias')]
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for key, shape, kind in sorted(specs):
        if kind == 'conv':
            a = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[2] * shape[3] * shape[0]))
        elif kind in ('bn_w', 'bn_v'):
            a = rng.uniform(0.5, 1.5, shape)
        elif kind == 'temporal':
            a = rng.standard_normal(shape) * 0.5
        elif kind == 'fc':
            a = rng.standard_normal(shape) * 0.05
        else:
            a = rng.standard_normal(shape) * 0.1
        sd[key] = np.ascontiguousarray(a, dtype=np.float32)
    return OrderedDict((k, sd[k]) for k, _s, _k in specs)


def remap_tdn_keys(state_dict: Mapping[str, object], num_class: int, depths=None) -> 'OrderedDict[str, object]':
    """A TDN checkpoint -> engine keys, which are the TSN module's own.  A ``state_dict`` wrapper is opened and a leading ``module.``
    (DataParallel) stripped; a key that is unknown as it stands but known without its ``.net`` components is renamed, as the
    reference's loader does (models/tdn.py:52-62).  ``base_model.conv1_temp.*`` and ``num_batches_tracked`` pass through (the engine
    ignores them); keys of neither spelling are dropped, as ``load_state_dict`` of the reference's merged dict drops them.
    A ``new_fc`` of another class count RAISES, naming both shapes: the reference would silently keep a random classifier."""
    if 'state_dict' in state_dict and isinstance(state_dict['state_dict'], Mapping):
        state_dict = state_dict['state_dict']
    known = {k for k, _s, _k in tdn_specs(depths)} | {'new_fc.weight', 'new_fc.bias', 'base_model.conv1_temp.weight', 'base_model.conv1_temp.bias'}
    out: 'OrderedDict[str, object]' = OrderedDict()
    for k, v in state_dict.items():
        name = k[len('module.'):] if k.startswith('module.') else k
        if name not in known and name.replace('.net', '') in known:
            name = name.replace('.net', '')
        if name in known or name.endswith('num_batches_tracked'):
            out[name] = v
    want = (int(num_class), R50_PLANES[-1] * EXPANSION)
    if 'new_fc.weight' in out and tuple(out['new_fc.weight'].shape) != want:
        raise ValueError(f'new_fc.weight of the checkpoint is {list(out["new_fc.weight"].shape)}, the model needs {list(want)}: '
                         'a classifier of another class count is not loaded')
    return out


def make_state_dict(seed: int = 0, num_class: int = 12, base_model: str = 'resnet50',
                    shift_place: str = 'blockres', non_local: bool = False, depths=None) -> 'OrderedDict[str, np.ndarray]':
    """Deterministic fp32 state dict (numpy arrays, torch layouts: conv OIHW, fc [cls, 2048] -- [cls, 512] for R18/R34).

    He-normal convs; BN statistics are all non-trivial so the fold is exercised; the last BN of
    each residual branch (bn3 of a Bottleneck, bn2 of a BasicBlock) is damped so activations stay O(1)
    through 16 blocks; the classifier uses std 0.05 (the reference's init std 0.001, tsm.py:260-262,
    gives logits too flat to discriminate between clips).  R50 draws the same stream as it always has
    (tests/golden/tsm_r50_logits.json depends on it); every other backbone draws its own shapes from the same procedure.  ``shift_place`` changes the keys only (``conv_specs``): one seed
    gives the same numbers under both spellings.
    ``non_local=True`` adds the ``nl.*`` tensors from a SECOND generator seeded from ``(seed, "nl")``, after everything else:
    every other key keeps its numbers.  theta / phi std ``NL_GAINS`` / sqrt(C) (soft but not uniform attention at the test
    sizes), g std 1 / sqrt(C), W.0 std 1 / sqrt(d), biases std 0.1; W.1 like every other BatchNorm with gamma damped by 0.35 -- NOT the zero
    of the original init, under which the block is the identity.
    ``base_model='convnext_base'``: timm's keys from a generator of its own (``_make_convnext_state_dict``), ``depths`` blocks per
    stage ((3, 3, 27, 3) by default); ``depths`` goes with no other backbone.
    """
    if is_convnext(base_model):
        return _make_convnext_state_dict(seed, num_class, depths)
    if depths is not None:
        raise ValueError(f'depths= goes with base_model={CONVNEXT!r} only')
    last_bn = '.bn2' if _backbone(base_model)[1] == 'basic' else '.bn3'
    rng = np.random.default_rng(seed)
    sd: 'OrderedDict[str, np.ndarray]' = OrderedDict()

    def f32(a):
        return np.ascontiguousarray(a, dtype=np.float32)

    for wkey, bnp, cout, cin, k in conv_specs(base_model, shift_place, non_local):
        fan_in = cin * k * k
        sd[wkey] = f32(rng.standard_normal((cout, cin, k, k)) * np.sqrt(2.0 / fan_in))
        damp = 0.35 if bnp.endswith(last_bn) else 1.0
        sd[bnp + '.weight'] = f32(rng.uniform(0.8, 1.2, cout) * damp)
        sd[bnp + '.bias'] = f32(rng.standard_normal(cout) * 0.1)
        sd[bnp + '.running_mean'] = f32(rng.standard_normal(cout) * 0.1)
        sd[bnp + '.running_var'] = f32(rng.uniform(0.6, 1.4, cout))
    sd['fc.weight'] = f32(rng.standard_normal((num_class, feature_width(base_model))) * 0.05)
    sd['fc.bias'] = f32(rng.standard_normal(num_class) * 0.1)
    if non_local:
        nl = np.random.default_rng([seed, int.from_bytes(b'nl', 'big')])
        for (p, c, d), lb in zip(nonlocal_specs(base_model), NL_BLOCKS):
            for name, cout, cin, std in (('.theta', d, c, NL_GAINS[lb] / np.sqrt(c)), ('.phi.0', d, c, NL_GAINS[lb] / np.sqrt(c)),
                                         ('.g.0', d, c, 1.0 / np.sqrt(c)), ('.W.0', c, d, 1.0 / np.sqrt(d))):
                sd[p + name + '.weight'] = f32(nl.standard_normal((cout, cin, 1, 1, 1)) * std)
                sd[p + name + '.bias'] = f32(nl.standard_normal(cout) * 0.1)
            sd[p + '.W.1.weight'] = f32(nl.uniform(0.8, 1.2, c) * 0.35)
            sd[p + '.W.1.bias'] = f32(nl.standard_normal(c) * 0.1)
            sd[p + '.W.1.running_mean'] = f32(nl.standard_normal(c) * 0.1)
            sd[p + '.W.1.running_var'] = f32(nl.uniform(0.6, 1.4, c))
    return sd


def remap_checkpoint_keys(state_dict: Mapping[str, object], num_class: int,
                          base_model: str = 'resnet50', non_local: bool = False,
                          temporal_pool: bool = False) -> 'OrderedDict[str, object]':
    """Checkpoint ``state_dict`` (``module.``/``model.``-prefixed) -> engine keys, exactly as create_model does it
    (models/tsm.py:451-473; pinned by tests/golden/ref_ckpt_remap.json, produced by executing those statements):
    the LAST TWO entries are the classifier; they become ``fc.weight`` / ``fc.bias`` iff the weight has ``num_class``
    rows and are dropped otherwise; every key loses its first dotted component.  Like the reference, a classifier
    that is already called ``module.fc`` is dropped by the delete that follows the copy -- the reference then keeps
    its random-init fc (``strict=False``); the engine reports the missing ``fc.weight`` instead of guessing.
    The rule does not depend on the backbone; ``base_model`` is checked to be one the engine implements.
    ``non_local=True``: a TSM-NL checkpoint's ``layerL.B.block.*`` / ``layerL.B.nl.*`` keys pass through the same rule (they are
    the engine's spelling already); a checkpoint without any ``.nl.`` key is refused here, by name, rather than at the
    engine's first missing tensor.  mmaction2's NL spelling is not mapped.
    ``temporal_pool=True``: TemporalPool holds layer2 as ``net``, so a temporal-pool checkpoint spells the stage's keys
    ``base_model.layer2.net.<b>.<rest>`` (``layer2.net.<b>.net.<rest>`` under block placement); the wrapper's ``net.`` is dropped,
    which gives the engine's keys.  A checkpoint with plain ``layer2.<b>.`` keys passes unchanged."""
    _backbone(base_model)
    if _non_local(non_local, base_model) and not any('.nl.' in k for k in state_dict):
        raise KeyError('non_local=True, but the checkpoint has no non-local block tensors (no ".nl." key)')
    items = OrderedDict(state_dict)
    keys = list(items.keys())
    fc_w, fc_b = keys[-2], keys[-1]
    if items[fc_w].shape[0] == num_class:
        items['module.fc.weight'] = items[fc_w]
        items['module.fc.bias'] = items[fc_b]
    del items[fc_w]
    del items[fc_b]
    out = OrderedDict(('.'.join(k.split('.')[1:]), v) for k, v in items.items())
    if temporal_pool:
        wrapped = 'base_model.layer2.net.'
        out = OrderedDict((('base_model.layer2.' + k[len(wrapped):]) if k.startswith(wrapped) else k, v) for k, v in out.items())
    return out


def remap_torchvision_keys(state_dict: Mapping[str, object]) -> 'OrderedDict[str, object]':
    """A plain torchvision ResNet ``state_dict`` (``conv1.weight``, ``bn1.*``, ``layer1.0.conv1.weight``, ..., ``fc.*``: the
    image model, image_classification.py:214 -- ``resnet18`` with a replaced ``fc``) -> engine keys: the backbone under
    ``base_model.``, ``fc.*`` as it is.  A Lightning ``state_dict`` carries one leading component on every key
    (``model.conv1.weight``): it is stripped when every key has the same one and ``conv1.weight`` is not already there.
    ``num_batches_tracked`` buffers pass through (the engine ignores them); anything else that is not a ResNet key raises."""
    keys = list(state_dict.keys())
    if not keys:
        raise ValueError('empty state dict')
    strip = 0
    if 'conv1.weight' not in state_dict:
        heads = {k.split('.', 1)[0] for k in keys}
        if len(heads) != 1 or f'{next(iter(heads))}.conv1.weight' not in state_dict:
            raise ValueError('not a torchvision ResNet state dict: no conv1.weight, with or without one leading component')
        strip = len(next(iter(heads))) + 1
    out: 'OrderedDict[str, object]' = OrderedDict()
    for k, v in state_dict.items():
        name = k[strip:]
        head = name.split('.', 1)[0]
        if head == 'fc':
            out[name] = v
        elif head in ('conv1', 'bn1') or (head.startswith('layer') and head[5:].isdigit()):
            out['base_model.' + name] = v
        else:
            raise ValueError(f'{k}: not a key of a torchvision ResNet')
    return out


def is_mmaction_state_dict(state_dict: Mapping[str, object]) -> bool:
    """mmaction2 ``Recognizer2D`` checkpoints (the reference's ``--mmlab`` branch, utils/inference_count.py:516-519,
    configs/tsm_MultiActionRepCount_sthv2.py:5-22) name their parts ``backbone.*`` / ``cls_head.*``."""
    return any(k.startswith('backbone.') for k in state_dict) and any(k.startswith('cls_head.') for k in state_dict)


def remap_mmaction_keys(state_dict: Mapping[str, object]) -> 'OrderedDict[str, object]':
    """mmaction2 0.24 ``ResNetTSM`` + ``TSMHead`` keys -> engine keys.

    mmaction builds every conv as a ``ConvModule`` (``.conv`` + ``.bn``) and wraps ``conv1.conv`` of each block in
    ``TemporalShift`` (``.net``): ``backbone.layer1.0.conv1.conv.net.weight`` -> ``base_model.layer1.0.conv1.net.weight``,
    ``backbone.layer1.0.conv1.bn.*`` -> ``base_model.layer1.0.bn1.*``, ``downsample.conv/bn`` -> ``downsample.0/1``,
    stem ``backbone.conv1.conv/bn`` -> ``base_model.conv1`` / ``base_model.bn1``, ``cls_head.fc_cls`` -> ``fc``.
    Same graph as the reference's own TSM (pytorch-style ResNet-50: stride on the 3x3; blockres shift, shift_div 8).
    ``ResNetTSM(shift_place='block')`` wraps each block whole, ``.net`` after the block index:
    ``backbone.layer1.0.net.conv1.conv.weight`` -> ``base_model.layer1.0.net.conv1.weight`` (and so on for every key of the block)."""
    out: 'OrderedDict[str, object]' = OrderedDict()
    for k, v in state_dict.items():
        if k.startswith('cls_head.fc_cls.'):
            out['fc.' + k[len('cls_head.fc_cls.'):]] = v
            continue
        if not k.startswith('backbone.'):
            continue                                    # e.g. optimizer-side buffers
        parts = k[len('backbone.'):].split('.')
        if parts[0] == 'conv1':                         # stem ConvModule
            tail = parts[2:]
            name = ['conv1'] + tail if parts[1] == 'conv' else ['bn1'] + tail
        elif parts[0].startswith('layer'):
            wrap = ['net'] if parts[2] == 'net' else []          # block placement: the whole block is wrapped
            if wrap:
                parts = parts[:2] + parts[3:]
            layer, blk, mod, kind, tail = parts[0], parts[1], parts[2], parts[3], parts[4:]
            if mod == 'downsample':
                name = [layer, blk] + wrap + ['downsample', '0' if kind == 'conv' else '1'] + tail
            elif kind == 'conv':
                name = [layer, blk] + wrap + [mod] + tail         # keeps a leading 'net' for the shifted conv1
            else:
                name = [layer, blk] + wrap + ['bn' + mod[-1]] + tail
        else:
            continue
        out['base_model.' + '.'.join(name)] = v
    return out


def required_keys(num_class_known: bool = True, base_model: str = 'resnet50', shift_place: str = 'blockres',
                  non_local: bool = False) -> Iterable[str]:
    for wkey, bnp, *_ in conv_specs(base_model, shift_place, non_local):
        yield wkey
        for s in ('.weight', '.bias', '.running_mean', '.running_var'):
            yield bnp + s
    if non_local:
        yield from nonlocal_keys(base_model)
    yield 'fc.weight'
    yield 'fc.bias'


def to_torch(sd: Mapping[str, np.ndarray]) -> Dict[str, 'object']:
    import torch
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}
