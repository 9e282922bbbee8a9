"""TSM-Wide-ResNet-50-2 test helpers: the CPU reference under both shift placements, and a width-parametrised nn.Module
for EXPORT tests.

The oracle needs no change for WRN-50-2: ``tsm_oracle.bottleneck`` / ``_bottleneck_bf16`` take every shape from the state
dict and ``trunk`` walks R50's (3, 4, 6, 3), so ``tsm_forward`` / ``tsm_forward_bf16`` compute WRN-50-2 from a WRN state
dict, and ``_block_place_ref.forward(..., 'resnet50')`` does the same for block placement.  The module follows
torchvision's Bottleneck with ``width_per_group``: conv1 / conv2 are ``planes * width / 64`` wide, conv3 and the
downsample ``planes * 4``; the module tree is ``tests/_torch_tsm.TorchTSM``'s, so ``state_dict()`` keys are R50's."""
from typing import Dict, Optional

import torch
import torch.nn as nn

from oracle import tsm_oracle
from oracle.tsm_oracle import EXPANSION, R50_BLOCKS, R50_PLANES
from tests._torch_tsm import _Shifted


@torch.no_grad()
def forward(sd: Dict[str, torch.Tensor], x: torch.Tensor, n_segment: int = 8, shift_div: int = 8, is_shift: bool = True,
            shift_place: str = 'blockres', taps: Optional[Dict[str, torch.Tensor]] = None,
            bf16: bool = False) -> torch.Tensor:
    """Logits of TSM-``sd`` (any Bottleneck width) on [B, T, 3, H, W]; ``bf16``: the bf16-storage restatement."""
    if shift_place == 'block':
        from tests import _block_place_ref
        return _block_place_ref.forward(sd, x, 'resnet50', n_segment=n_segment, shift_div=shift_div, is_shift=is_shift,
                                        taps=taps, bf16=bf16)
    fwd = tsm_oracle.tsm_forward_bf16 if bf16 else tsm_oracle.tsm_forward
    return fwd(sd, x, n_segment=n_segment, shift_div=shift_div, is_shift=is_shift, taps=taps)


class _WideBottleneck(nn.Module):
    def __init__(self, cin, planes, width, stride, down, n_segment, fold_div):
        super().__init__()
        mid = planes * width // 64
        self.conv1 = _Shifted(nn.Conv2d(cin, mid, 1, bias=False), n_segment, fold_div)
        self.bn1 = nn.BatchNorm2d(mid)
        self.conv2 = nn.Conv2d(mid, mid, 3, stride, 1, bias=False)
        self.bn2 = nn.BatchNorm2d(mid)
        self.conv3 = nn.Conv2d(mid, planes * EXPANSION, 1, bias=False)
        self.bn3 = nn.BatchNorm2d(planes * EXPANSION)
        self.relu = nn.ReLU(inplace=True)
        self.downsample = nn.Sequential(nn.Conv2d(cin, planes * EXPANSION, 1, stride, bias=False),
                                        nn.BatchNorm2d(planes * EXPANSION)) if down else None

    def forward(self, x):
        out = self.relu(self.bn1(self.conv1(x)))
        out = self.relu(self.bn2(self.conv2(out)))
        out = self.bn3(self.conv3(out))
        identity = x if self.downsample is None else self.downsample(x)
        return self.relu(out + identity)


class _WideTrunk(nn.Module):
    def __init__(self, width, n_segment, fold_div):
        super().__init__()
        self.conv1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False)
        self.bn1 = nn.BatchNorm2d(64)
        self.relu = nn.ReLU(inplace=True)
        self.maxpool = nn.MaxPool2d(3, 2, 1)
        cin = 64
        for li, (nb, planes) in enumerate(zip(R50_BLOCKS, R50_PLANES), start=1):
            blocks = []
            for b in range(nb):
                blocks.append(_WideBottleneck(cin, planes, width, 2 if (b == 0 and li > 1) else 1, b == 0, n_segment,
                                              fold_div))
                cin = planes * EXPANSION
            setattr(self, f'layer{li}', nn.Sequential(*blocks))
        self.avgpool = nn.AdaptiveAvgPool2d(1)

    def forward(self, x):
        x = self.maxpool(self.relu(self.bn1(self.conv1(x))))
        x = self.layer4(self.layer3(self.layer2(self.layer1(x))))
        return self.avgpool(x).flatten(1)


class TorchWideTSM(nn.Module):
    """TSM over a torchvision-style ResNet-50 with ``width_per_group = width`` (64: R50, 128: WRN-50-2)."""

    def __init__(self, width=128, num_class=12, n_segment=8, fold_div=8):
        super().__init__()
        self.n_segment = n_segment
        self.base_model = _WideTrunk(width, n_segment, fold_div)
        self.new_fc = nn.Linear(512 * EXPANSION, num_class)

    def forward(self, x):
        x = x.view((-1,) + tuple(x.shape[-3:]))
        out = self.new_fc(self.base_model(x))
        out = out.view(-1, self.n_segment, out.shape[-1])
        return out.mean(dim=1, keepdim=True).squeeze(1)

    def load_engine_state_dict(self, sd):
        """Engine / oracle keys (``fc.*``) -> this module's (``new_fc.*``); strict."""
        missing, unexpected = self.load_state_dict({k.replace('fc.', 'new_fc.') if k.startswith('fc.') else k: torch.as_tensor(v)
                                                    for k, v in sd.items()}, strict=False)
        assert not unexpected and all(k.endswith('num_batches_tracked') for k in missing), (missing, unexpected)
        return self

    def engine_state_dict(self):
        return {k.replace('new_fc.', 'fc.'): v for k, v in self.state_dict().items() if not k.endswith('num_batches_tracked')}
