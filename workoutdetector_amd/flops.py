"""Algorithmic work of the TSM-ResNet forward: per-layer GEMM shapes and MACs.

Used by ``bench.py`` (roofline accounting) and ``tools/``; derived from ``weights.block_specs()`` and the spatial
schedule of ResNet-50 v1.5 / Wide-ResNet-50-2 (7x7 s2 stem, 3x3 s2 max-pool, stride on the 3x3 of each stage's first block) or of
ResNet-18 / 34 (BasicBlock: stride on conv1).
Shift, BN fold, ReLU, pooling and the segment mean count zero FLOPs.
"""
from __future__ import annotations

from typing import Dict, List

from .weights import STEM, block_specs, feature_width


def _out(size: int, k: int, stride: int) -> int:
    return (size + 2 * (k // 2) - k) // stride + 1


def layer_table(height: int = 224, width: int = 224, base_model: str = 'resnet50') -> List[Dict[str, int]]:
    """One row per conv launch-able layer: name, cin, cout, k, s (stride), m (output pixels per frame), macs per frame."""
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


def macs_per_frame(height: int = 224, width: int = 224, num_class: int = 12, base_model: str = 'resnet50') -> int:
    return sum(r['macs'] for r in layer_table(height, width, base_model)) + feature_width(base_model) * num_class


def flops_per_clip(num_segments: int = 8, height: int = 224, width: int = 224, num_class: int = 12,
                   base_model: str = 'resnet50') -> float:
    return 2.0 * macs_per_frame(height, width, num_class, base_model) * num_segments
