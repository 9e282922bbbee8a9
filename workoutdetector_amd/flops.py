"""Algorithmic work of the TSM-ResNet forward: per-layer GEMM shapes and MACs.

Used by ``bench.py`` (roofline accounting) and ``tools/``; derived from ``weights.block_specs()`` and the spatial
schedule of ResNet-50 v1.5 / Wide-ResNet-50-2 (7x7 s2 stem, 3x3 s2 max-pool, stride on the 3x3 of each stage's first block) or of
ResNet-18 / 34 (BasicBlock: stride on conv1).
Shift, BN fold, ReLU, pooling and the segment mean count zero FLOPs.
"""
from __future__ import annotations

from typing import Dict, List

from .weights import CONVNEXT_WIDTHS, NL_BLOCKS, STEM, _convnext_depths, block_specs, feature_width, is_convnext, nonlocal_specs


def _out(size: int, k: int, stride: int) -> int:
    return (size + 2 * (k // 2) - k) // stride + 1


def convnext_table(height: int = 224, width: int = 224, depths=None) -> List[Dict[str, int]]:
    """``convnext_base``'s rows, the same columns as ``layer_table``: the stem (4x4 at stride 4 over 3 channels), per stage its
    downsample (2x2 at stride 2, floor mode) and per block the depthwise 7x7 (``cin`` = 1: one input channel per output), fc1 and
    fc2.  LayerNorm, GELU, the layer scale and the pooling count zero MACs.  15.4 GMAC per 224 x 224 frame with the 1000-class
    head (``macs_per_frame``)."""
    h, w = height // 4, width // 4
    c0 = CONVNEXT_WIDTHS[0]
    rows: List[Dict[str, int]] = [dict(name='stem', cin=3, cout=c0, k=4, s=4, m=h * w, macs=h * w * c0 * 3 * 16)]
    for s, (nb, c) in enumerate(zip(_convnext_depths(depths), CONVNEXT_WIDTHS)):
        if s > 0:
            h, w = h // 2, w // 2
            rows.append(dict(name=f'stages.{s}.downsample', cin=c // 2, cout=c, k=2, s=2, m=h * w, macs=h * w * c * (c // 2) * 4))
        for b in range(nb):
            p = f'stages.{s}.blocks.{b}'
            rows.append(dict(name=p + '.conv_dw', cin=1, cout=c, k=7, s=1, m=h * w, macs=h * w * c * 49))
            rows.append(dict(name=p + '.fc1', cin=c, cout=4 * c, k=1, s=1, m=h * w, macs=h * w * c * 4 * c))
            rows.append(dict(name=p + '.fc2', cin=4 * c, cout=c, k=1, s=1, m=h * w, macs=h * w * c * 4 * c))
    return rows


def layer_table(height: int = 224, width: int = 224, base_model: str = 'resnet50') -> List[Dict[str, int]]:
    """One row per conv launch-able layer: name, cin, cout, k, s (stride), m (output pixels per frame), macs per frame."""
    if is_convnext(base_model):
        return convnext_table(height, width)
    _wkey, _bn, cout, cin, k = STEM
    ho, wo = _out(height, k, 2), _out(width, k, 2)
    rows: List[Dict[str, int]] = [dict(name='conv1', cin=cin, cout=cout, k=k, s=2, m=ho * wo, macs=ho * wo * cout * cin * k * k)]
    h, w = _out(ho, 3, 2), _out(wo, 3, 2)                  # max-pool
    for li, b, stride, convs in block_specs(base_model):
        ho, wo = _out(h, 3, stride), _out(w, 3, stride)    # the block's output size: its one strided 3x3 sets it
        for role, cout, cin, k, s, at_input in convs:
            hi, wi = (h, w) if at_input else (ho, wo)
            m = _out(hi, k, s) * _out(wi, k, s)
            rows.append(dict(name=f'layer{li}.{b}.{role}', cin=cin, cout=cout, k=k, s=s, m=m, macs=m * cout * cin * k * k))
        h, w = ho, wo
    return rows


def tdn_table(height: int = 224, width: int = 224, depths=None) -> List[Dict[str, int]]:
    """TDN-ResNet50's rows per SEGMENT (five input frames), the same columns as ``layer_table``: the trunk's stem, conv1_5 (its 588
    real K values, not the padded 1024 of its GEMM), resnext_layer1's and layer1's Bottlenecks and the BottleneckShift blocks of
    layers 2-4, each with its long-term module: the squeeze (C -> r = C / 16), the depthwise 3x3 (``cin`` = 1), the two full 3x3
    r -> r convs for both directions (``smallscale2`` on the pooled map), the excite (r -> C, both directions) and the 3-tap
    temporal conv.  Differences, pools, blends, the sigmoid and BatchNorm count zero MACs."""
    from .weights import EXPANSION, R50_PLANES, _tdn_depths
    d = _tdn_depths(depths)
    h1, w1 = _out(height, 7, 2), _out(width, 7, 2)
    rows: List[Dict[str, int]] = [dict(name='conv1', cin=3, cout=64, k=7, s=2, m=h1 * w1, macs=h1 * w1 * 64 * 3 * 49)]
    h5, w5 = _out(height // 2, 7, 2), _out(width // 2, 7, 2)
    rows.append(dict(name='diff.conv1_5', cin=12, cout=64, k=7, s=2, m=h5 * w5, macs=h5 * w5 * 64 * 12 * 49))
    for li in range(0, 5):      # 0: resnext_layer1, on the maps of xd0
        stage = max(li, 1) - 1
        planes, cout = R50_PLANES[stage], R50_PLANES[stage] * EXPANSION
        cin = 64 if stage == 0 else R50_PLANES[stage - 1] * EXPANSION
        if li == 0:
            h, w = _out(h5, 3, 2), _out(w5, 3, 2)
        elif li == 1:
            h, w = _out(h1, 3, 2), _out(w1, 3, 2)
        for b in range(d[stage]):
            p = f'resnext_layer1.{b}' if li == 0 else f'layer{li}.{b}'
            s = 2 if (b == 0 and stage > 0) else 1
            ho, wo = _out(h, 3, s), _out(w, 3, s)
            rows.append(dict(name=p + '.conv1', cin=cin, cout=planes, k=1, s=1, m=h * w, macs=h * w * planes * cin))
            if li >= 2:
                r, mp = planes // 16, (h // 2) * (w // 2)
                rows.append(dict(name=p + '.mse.conv1', cin=planes, cout=r, k=1, s=1, m=h * w, macs=h * w * r * planes))
                rows.append(dict(name=p + '.mse.conv2', cin=1, cout=r, k=3, s=1, m=h * w, macs=h * w * r * 9))
                rows.append(dict(name=p + '.mse.conv3_smallscale2', cin=r, cout=r, k=3, s=1, m=2 * mp, macs=2 * mp * r * r * 9))
                rows.append(dict(name=p + '.mse.conv3_smallscale4', cin=r, cout=r, k=3, s=1, m=2 * h * w, macs=2 * h * w * r * r * 9))
                rows.append(dict(name=p + '.mse.conv3', cin=r, cout=planes, k=1, s=1, m=2 * h * w, macs=2 * h * w * planes * r))
                rows.append(dict(name=p + '.shift.conv', cin=1, cout=planes, k=3, s=1, m=h * w, macs=h * w * planes * 3, one_d=True))      # (3 taps over time)
            rows.append(dict(name=p + '.conv2', cin=planes, cout=planes, k=3, s=s, m=ho * wo, macs=ho * wo * planes * planes * 9))
            rows.append(dict(name=p + '.conv3', cin=planes, cout=cout, k=1, s=1, m=ho * wo, macs=ho * wo * cout * planes))
            if b == 0:
                rows.append(dict(name=p + '.downsample', cin=cin, cout=cout, k=1, s=s, m=ho * wo, macs=ho * wo * cout * cin))
            cin, h, w = cout, ho, wo
    return rows


def tdn_flops_per_clip(num_segments: int = 8, height: int = 224, width: int = 224, num_class: int = 12, depths=None) -> float:
    """FLOPs of one TDN clip: ``tdn_table`` and the classifier, per segment, times ``num_segments``."""
    return 2.0 * num_segments * (sum(r['macs'] for r in tdn_table(height, width, depths)) + 2048 * num_class)


def macs_per_frame(height: int = 224, width: int = 224, num_class: int = 12, base_model: str = 'resnet50') -> int:
    return sum(r['macs'] for r in layer_table(height, width, base_model)) + feature_width(base_model) * num_class


def _stage_size(size: int, layer: int) -> int:
    """Side of layer<layer>'s output: the stem, the max-pool, then one strided 3x3 per stage from layer2 on."""
    s = _out(_out(size, 7, 2), 3, 2)
    for _ in range(layer - 1):
        s = _out(s, 3, 2)
    return s


def nonlocal_table(num_segments: int = 8, height: int = 224, width: int = 224, base_model: str = 'resnet50') -> List[Dict[str, int]]:
    """One row per non-local block (``create_model(non_local=True)``): name, c, d = c // 2, nq = T * H * W, nk = T * (H // 2) *
    (W // 2) and the MACs PER CLIP of its 1x1 convs (theta | phi | g: nq * c * 3 d, W: nq * d * c) and of the attention (the
    scores nq * nk * d, P V the same again).  The pool and the softmax count zero FLOPs."""
    rows = []
    for (li, b), (_prefix, c, d) in zip(NL_BLOCKS, nonlocal_specs(base_model)):      # (raises for a BasicBlock backbone)
        h, w = _stage_size(height, li), _stage_size(width, li)
        nq, nk = num_segments * h * w, num_segments * (h // 2) * (w // 2)
        rows.append(dict(name=f'layer{li}.{b}.nl', c=c, d=d, nq=nq, nk=nk, conv_macs=nq * (c * 3 * d + d * c), attn_macs=2 * nq * nk * d))
    return rows


def flops_per_clip(num_segments: int = 8, height: int = 224, width: int = 224, num_class: int = 12,
                   base_model: str = 'resnet50', non_local: bool = False, temporal_pool: bool = False) -> float:
    """``temporal_pool=True`` (``create_model(temporal_pool=True)``): the stem and layer1 run on all ``num_segments`` frames of a
    clip, layers 2-4 and the classifier on the ``num_segments // 2`` frames the pool leaves; the pool itself counts zero FLOPs.
    ``base_model='tdn_resnet50'``: ``tdn_flops_per_clip`` (full depth)."""
    if base_model == 'tdn_resnet50':
        if non_local or temporal_pool:
            raise ValueError('tdn_resnet50 has no non_local / temporal_pool')
        return tdn_flops_per_clip(num_segments, height, width, num_class)
    nl =sum(r['conv_macs'] + r['attn_macs'] for r in nonlocal_table(num_segments, height, width, base_model)) if non_local else 0
    if not temporal_pool:
        return 2.0 * (macs_per_frame(height, width, num_class, base_model) * num_segments + nl)
    if non_local or num_segments <= 0 or num_segments % 2:
        raise ValueError('temporal_pool=True needs an even num_segments and excludes non_local=True')
    rows = layer_table(height, width, base_model)
    pooled = sum(r['macs'] for r in rows if r['name'].startswith(('layer2.', 'layer3.', 'layer4.'))) + feature_width(base_model) * num_class
    full = sum(r['macs'] for r in rows if not r['name'].startswith(('layer2.', 'layer3.', 'layer4.')))
    return 2.0 * (full * num_segments + pooled * (num_segments // 2))
