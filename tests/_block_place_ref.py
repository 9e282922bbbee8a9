"""CPU reference of the block placement of the temporal shift (``shift_place='block'``, workoutdetector/models/tsm.py:104-124),
built from ``oracle.tsm_oracle``'s and ``tests._basicblock_ref``'s own block functions, and an nn.Module spelling of the same
network for key / export tests.

Test infrastructure, like oracle/.  Every block of layer1-4 is wrapped whole: ``TemporalShift(block)(x) = block(shift(x))``.
So per block

    xs = temporal_shift(x);  out = <the blockres block function with is_shift=False>(xs)

which makes conv1, the identity and the downsample all read ``xs``.  The shift is pure data movement, so composing it this
way is exact in every storage format (fp32, bf16-storage).  State-dict keys are the wrapped spelling
``base_model.layerL.B.net.<name>``; the stem and the fc keep theirs.
"""
from typing import Dict, Optional

import torch
import torch.nn as nn

from oracle import tsm_oracle
from oracle.tsm_oracle import R50_BLOCKS, head, stem, temporal_shift
from tests import _basicblock_ref as basic
from tests._torch_tsm import TorchTSM, _Shifted

BLOCKS = {'resnet50': R50_BLOCKS, **basic.BLOCKS}


def _block_fn(base_model, bf16):
    if base_model == 'resnet50':
        fn = tsm_oracle._bottleneck_bf16 if bf16 else tsm_oracle.bottleneck
        return lambda x, sd, prefix, stride, T, div, taps, name: fn(x, sd, prefix, stride, T, div, False)
    fn = basic.basic_block_bf16 if bf16 else basic.basic_block
    return lambda x, sd, prefix, stride, T, div, taps, name: fn(x, sd, prefix, stride, T, div, False, taps, name)


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, base_model: str = 'resnet50', n_segment: int = 8,
            shift_div: int = 8, is_shift: bool = True, taps: Optional[Dict[str, torch.Tensor]] = None,
            bf16: bool = False) -> torch.Tensor:
    """x: [B*T,3,H,W] or [B,T,3,H,W] fp32 -> logits [B,num_class]; ``sd`` in the block spelling (``layerL.B.net.*``).
    ``taps`` collects 'stem', 'layerL.B' (NCHW), for BasicBlocks also 'layerL.B.conv1', and 'logits'.  ``bf16``: the
    bf16-storage restatement (the engine's bf16 mode)."""
    if x.dim() == 5:
        x = x.reshape((-1,) + tuple(x.shape[2:]))
    x = x.to(torch.float32)
    if bf16:
        h = tsm_oracle.conv_bn_act_bf16(x, sd['base_model.conv1.weight'], tsm_oracle._sd_bn(sd, 'base_model.bn1'), 2, 3,
                                        True, round_output=True)
        h = torch.nn.functional.max_pool2d(h, kernel_size=3, stride=2, padding=1)
    else:
        h = stem(x, sd)
    if taps is not None:
        taps['stem'] = h
    block = _block_fn(base_model, bf16)
    for li, nb in enumerate(BLOCKS[base_model], start=1):
        for b in range(nb):
            name = f'layer{li}.{b}'
            xs = temporal_shift(h, n_segment, shift_div) if is_shift else h
            h = block(xs, sd, f'base_model.{name}.net', 2 if (b == 0 and li > 1) else 1, n_segment, shift_div, taps, name)
            if taps is not None:
                taps[name] = h
    out = head(h, sd, n_segment)
    if taps is not None:
        taps['logits'] = out
    return out


def as_block_keys(sd):
    """A blockres-spelled state dict (``layerL.B.conv1.net.weight``, ``layerL.B.bn1.*``) in the block spelling."""
    out = {}
    for k, v in sd.items():
        parts = k.split('.')
        if len(parts) > 3 and parts[0] == 'base_model' and parts[1].startswith('layer'):
            parts = parts[:3] + ['net'] + [p for p in parts[3:] if p != 'net']
        out['.'.join(parts)] = v
    return out


# ---- nn.Module spelling: TSM(shift_place='block') wraps each block as `.net` -------------------------------------------
def torch_block_tsm(base_model='resnet50', num_class=12, n_segment=8, fold_div=8):
    """The reference module tree with every block of layer1-4 wrapped whole (``layerL.B.net.conv1.weight``, ...): the
    blockres tree of tests/_torch_tsm.py (R50) or tests/_basicblock_ref.py (R18 / R34) with conv1 unwrapped."""
    net = (TorchTSM(num_class, n_segment, fold_div) if base_model == 'resnet50'
           else basic.TorchBasicTSM(base_model, num_class, n_segment, fold_div))
    for li in range(1, 5):
        layer = getattr(net.base_model, f'layer{li}')
        for b in range(len(layer)):
            blk = layer[b]
            blk.conv1 = blk.conv1.net
            layer[b] = _Shifted(blk, n_segment, fold_div)
    return net
