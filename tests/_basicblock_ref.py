"""CPU reference of TSM-ResNet18 / 34 (torchvision BasicBlock, the temporal shift in front of every conv1), built from
``oracle.tsm_oracle``'s own pieces, and an nn.Module spelling of the same network for key / export tests.

Test infrastructure, like oracle/.  Semantics (workoutdetector/models/tsm.py:104-139 with torchvision's BasicBlock):

    out = relu(bn2(conv2(relu(bn1(conv1(shift(x))))))  +  identity)

conv1 is 3x3 at the block's stride, conv2 3x3 at stride 1; identity is the UNSHIFTED x, or downsample(x) (1x1 conv at
the stride + BN) in the first block of layers 2-4.  ``len(layer3) < 23`` for both depths, so every block is shifted.

The bf16 form rounds what the engine stores: the folded weights, conv1's output, the downsample output (its own launch)
and the block output; every sum accumulates in fp32.
"""
from typing import Dict, Optional

import torch
import torch.nn as nn
import torch.nn.functional as F

from oracle.tsm_oracle import (_bn, _conv1_key, _sd_bn, bf16_round, conv_bn_act_bf16, head, stem, temporal_shift)
from tests._torch_tsm import _Shifted

PLANES = (64, 128, 256, 512)
BLOCKS = {'resnet18': (2, 2, 2, 2), 'resnet34': (3, 4, 6, 3)}


def _blocks(base_model):
    for li, nb in enumerate(BLOCKS[base_model], start=1):
        for b in range(nb):
            yield li, b, (2 if (b == 0 and li > 1) else 1)


def basic_block(x, sd, prefix, stride, n_segment, shift_div, is_shift=True, taps=None, name=''):
    h = temporal_shift(x, n_segment, shift_div) if is_shift else x
    h = F.relu(_bn(F.conv2d(h, sd[_conv1_key(sd, prefix)], stride=stride, padding=1), sd, prefix + '.bn1'))
    if taps is not None:
        taps[name + '.conv1'] = h
    h = _bn(F.conv2d(h, sd[prefix + '.conv2.weight'], padding=1), sd, prefix + '.bn2')
    identity = x
    if prefix + '.downsample.0.weight' in sd:
        identity = _bn(F.conv2d(x, sd[prefix + '.downsample.0.weight'], stride=stride), sd, prefix + '.downsample.1')
    return F.relu(h + identity)


def basic_block_bf16(x, sd, prefix, stride, n_segment, shift_div, is_shift=True, taps=None, name=''):
    h = temporal_shift(x, n_segment, shift_div) if is_shift else x
    h = conv_bn_act_bf16(h, sd[_conv1_key(sd, prefix)], _sd_bn(sd, prefix + '.bn1'), stride, 1, True, round_output=True)
    if taps is not None:
        taps[name + '.conv1'] = h
    identity = x
    if prefix + '.downsample.0.weight' in sd:
        identity = conv_bn_act_bf16(x, sd[prefix + '.downsample.0.weight'], _sd_bn(sd, prefix + '.downsample.1'), stride,
                                    0, False, round_output=True)
    return conv_bn_act_bf16(h, sd[prefix + '.conv2.weight'], _sd_bn(sd, prefix + '.bn2'), 1, 1, True,
                            residual=identity, round_output=True)


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, base_model: str, n_segment: int = 8, shift_div: int = 8,
            is_shift: bool = True, taps: Optional[Dict[str, torch.Tensor]] = None, bf16: bool = False) -> torch.Tensor:
    """x: [B*T,3,H,W] or [B,T,3,H,W] fp32 -> logits [B,num_class]; ``taps`` collects 'stem', 'layerL.B',
    'layerL.B.conv1' (NCHW) and 'logits'.  ``bf16``: the bf16-storage restatement."""
    if x.dim() == 5:
        x = x.reshape((-1,) + tuple(x.shape[2:]))
    x = x.to(torch.float32)
    if bf16:
        h = conv_bn_act_bf16(x, sd['base_model.conv1.weight'], _sd_bn(sd, 'base_model.bn1'), 2, 3, True,
                             round_output=True)
        h = F.max_pool2d(h, kernel_size=3, stride=2, padding=1)
    else:
        h = stem(x, sd)
    if taps is not None:
        taps['stem'] = h
    block = basic_block_bf16 if bf16 else basic_block
    for li, b, stride in _blocks(base_model):
        name = f'layer{li}.{b}'
        h = block(h, sd, 'base_model.' + name, stride, n_segment, shift_div, is_shift, taps, name)
        if taps is not None:
            taps[name] = h
    out = head(h, sd, n_segment)
    if taps is not None:
        taps['logits'] = out
    return out


# ---- nn.Module spelling (TSM.state_dict() names: conv1 wrapped as `.net`) ----------------------------------------------
class _BasicBlock(nn.Module):
    def __init__(self, cin, planes, stride, n_segment, fold_div):
        super().__init__()
        self.conv1 = _Shifted(nn.Conv2d(cin, planes, 3, stride, 1, bias=False), n_segment, fold_div)
        self.bn1 = nn.BatchNorm2d(planes)
        self.conv2 = nn.Conv2d(planes, planes, 3, 1, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(planes)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = (nn.Sequential(nn.Conv2d(cin, planes, 1, stride, bias=False), nn.BatchNorm2d(planes))
                           if (stride != 1 or cin != planes) else None)

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.bn2(self.conv2(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class _Trunk(nn.Module):
    def __init__(self, base_model, n_segment, fold_div):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for li, (nb, planes) in enumerate(zip(BLOCKS[base_model], PLANES), start=1):
            blocks = []
            for b in range(nb):
                blocks.append(_BasicBlock(cin, planes, 2 if (b == 0 and li > 1) else 1, n_segment, fold_div))
                cin = planes
            setattr(self, f'layer{li}', nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.avgpool(x).flatten(1)


class TorchBasicTSM(nn.Module):
    """TSM-R18 / R34 with the reference's module tree: ``base_model.*`` and ``new_fc`` [num_class, 512]."""

    def __init__(self, base_model='resnet18', num_class=12, n_segment=8, fold_div=8):
        super().__init__()
        self.n_segment = n_segment
        self.base_model = _Trunk(base_model, n_segment, fold_div)
        self.new_fc = nn.Linear(512, num_class)

    def forward(self, x):
        x = x.view((-1,) + tuple(x.shape[-3:]))
        out = self.new_fc(self.base_model(x))
        out = out.view(-1, self.n_segment, out.shape[-1])
        return out.mean(dim=1, keepdim=True).squeeze(1)

    def engine_state_dict(self):
        """This module's tensors under engine / oracle keys (``fc.*``; no num_batches_tracked)."""
        return {k.replace('new_fc.', 'fc.'): v.detach().clone() for k, v in self.state_dict().items()
                if not k.endswith('num_batches_tracked')}

    def load_engine_state_dict(self, sd):
        missing, unexpected = self.load_state_dict(
            {k.replace('fc.', 'new_fc.') if k.startswith('fc.') else k: torch.as_tensor(v) for k, v in sd.items()},
            strict=False)
        assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing), (missing, unexpected)
        return self
