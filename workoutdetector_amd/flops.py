"""Algorithmic work of the TSM-ResNet forward: per-layer GEMM shapes and MACs.

Used by ``bench.py`` (roofline accounting) and ``tools/``; derived from ``weights.conv_specs()`` and the spatial
schedule of ResNet-50 v1.5 / Wide-ResNet-50-2 (7x7 s2 stem, 3x3 s2 max-pool, stride on the 3x3 of each stage's first block) or of
ResNet-18 / 34 (BasicBlock: stride on conv1).
Shift, BN fold, ReLU, pooling and the segment mean count zero FLOPs.
"""
from __future__ import annotations

from typing import Dict, List

from .weights import conv_specs, feature_width


def _out(size: int, k: int, stride: int) -> int:
    return (size + 2 * (k // 2) - k) // stride + 1


def layer_table(height: int = 224, width: int = 224, base_model: str = 'resnet50') -> List[Dict[str, int]]:
    """One row per conv launch-able layer: name, cin, cout, k, s (stride), m (output pixels per frame), macs per frame."""
    rows: List[Dict[str, int]] = []
    h, w = height, width
    block_in = None          # spatial size at the input of the current block
    basic = feature_width(base_model) != 2048
    for wkey, _bn, cout, cin, k in conv_specs(base_model):
        name = wkey[len('base_model.'):].replace('.net.weight', '').replace('.0.weight', '').replace('.weight', '')
        if name == 'conv1':
            ho, wo = _out(h, 7, 2), _out(w, 7, 2)
            rows.append(dict(name=name, cin=cin, cout=cout, k=k, s=2, m=ho * wo, macs=ho * wo * cout * cin * k * k))
            h, w = _out(ho, 3, 2), _out(wo, 3, 2)          # max-pool
            continue
        layer, block, part = name.split('.')
        stride = 2 if (block == '0' and layer != 'layer1') else 1
        if basic and part == 'conv1':                      # BasicBlock: the stride sits on conv1
            block_in = (h, w)
            s, ho, wo = stride, _out(h, 3, stride), _out(w, 3, stride)
            h, w = ho, wo
        elif basic and part == 'conv2':
            s, ho, wo = 1, h, w
        elif part == 'conv1':
            block_in = (h, w)
            s, ho, wo = 1, h, w
        elif part == 'conv2':
            s, ho, wo = stride, _out(h, 3, stride), _out(w, 3, stride)
            h, w = ho, wo
        elif part == 'conv3':
            s, ho, wo = 1, h, w
        else:                                              # downsample: 1x1 strided on the block input
            s, ho, wo = stride, _out(block_in[0], 1, stride), _out(block_in[1], 1, stride)
        rows.append(dict(name=name, cin=cin, cout=cout, k=k, s=s, m=ho * wo, macs=ho * wo * cout * cin * k * k))
    return rows


def macs_per_frame(height: int = 224, width: int = 224, num_class: int = 12, base_model: str = 'resnet50') -> int:
    return sum(r['macs'] for r in layer_table(height, width, base_model)) + feature_width(base_model) * num_class


def flops_per_clip(num_segments: int = 8, height: int = 224, width: int = 224, num_class: int = 12,
                   base_model: str = 'resnet50') -> float:
    return 2.0 * macs_per_frame(height, width, num_class, base_model) * num_segments
