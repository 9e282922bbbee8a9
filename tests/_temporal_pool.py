"""Shared pieces of the temporal-pool tests (tests/test_temporal_pool_cpu.py, tests/test_temporal_pool_gpu.py).

* ``TemporalPool``: the wrapper of the TSM code base's make_temporal_pool, written from the operator's definition
  (include/tsm_hip.h, tsm_set_temporal_pool): it holds the wrapped stage as ``net`` and max-pools its input over time, kernel 3,
  stride 2, padding 1, per clip, before the stage runs.
* ``torch_tsm_tp``: ``tests._torch_tsm.TorchTSM`` with layer2 wrapped, every shift module of layers 2-4 and the model's own
  consensus set to T / 2 segments, the way make_temporal_shift's ``n_segment_list = [T, T/2, T/2, T/2]`` branch leaves it.
* ``run_with_taps``: one forward with forward hooks that record the engine's tap points as NHWC arrays.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

from tests._torch_tsm import TorchTSM, _Shifted
from workoutdetector_amd.weights import BACKBONES, WIDTHS

WRAPPED = 'base_model.layer2.'


class TemporalPool(nn.Module):
    def __init__(self, net, n_segment):
        super().__init__()
        self.net, self.n_segment = net, n_segment

    def pool(self, x):                                     # [B * T, C, H, W] -> [B * T / 2, C, H, W]
        nt, c, h, w = x.shape
        v = x.view(nt // self.n_segment, self.n_segment, c, h, w).transpose(1, 2)       # [B, C, T, H, W]
        v = F.max_pool3d(v, kernel_size=(3, 1, 1), stride=(2, 1, 1), padding=(1, 0, 0))
        return v.transpose(1, 2).reshape(nt // 2, c, h, w)

    def forward(self, x):
        return self.net(self.pool(x))


def wrapper_keys(sd):
    """Engine keys -> the wrapped module's: layer2's keys under the wrapper's ``net``."""
    return {(WRAPPED + 'net.' + k[len(WRAPPED):]) if k.startswith(WRAPPED) else k: v for k, v in sd.items()}


def last_block(base_model, layer):
    """Index of the last block of ``layer`` (1-based)."""
    return BACKBONES[base_model][0][layer - 1] - 1


def taps_of(base_model):
    """The tap points of the engine tests: layer1's last block, the pooled tensor, layer2.0, layer3.1 and layer4's last block
    (layer4.2; a BasicBlock resnet18's layer4 ends at layer4.1)."""
    return (f'layer1.{last_block(base_model, 1)}', 'layer2.tpool', 'layer2.0', 'layer3.1', f'layer4.{last_block(base_model, 4)}')


def torch_tsm_tp(base_model='resnet50', shift_place='blockres', num_class=12, n_segment=8, sd=None, dtype=torch.float64):
    """TorchTSM with the temporal pool; ``sd`` (engine keys) loaded strictly; eval mode, ``dtype``."""
    assert n_segment % 2 == 0
    net = TorchTSM(base_model, WIDTHS.get(base_model, 64), shift_place, num_class, n_segment)
    for li in (2, 3, 4):
        for m in getattr(net.base_model, f'layer{li}').modules():
            if isinstance(m, _Shifted):
                m.n_segment = n_segment // 2
    net.base_model.layer2 = TemporalPool(net.base_model.layer2, n_segment)
    net.n_segment = n_segment // 2                         # the consensus runs over the frames that are left
    if sd is not None:
        net.load_engine_state_dict(wrapper_keys(sd))
    return net.to(dtype).eval()


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


@torch.no_grad()
def run_with_taps(net, x, taps):
    """One forward of ``x`` [B, T, 3, H, W] through ``net`` (its dtype) -> (logits [B, num_class], per-segment logits
    [B, T / 2, num_class], pooled features [B * T / 2, feat], {tap: NHWC ndarray})."""
    got, handles = {}, []
    for name in taps:
        if name == 'layer2.tpool':                         # the wrapped stage's input
            handles.append(net.base_model.layer2.net.register_forward_pre_hook(
                lambda _m, inp, name=name: got.__setitem__(name, _nhwc(inp[0]))))
            continue
        layer, b = name.split('.')
        stage = getattr(net.base_model, layer)
        mod = (stage.net if isinstance(stage, TemporalPool) else stage)[int(b)]
        handles.append(mod.register_forward_hook(lambda _m, _i, out, name=name: got.__setitem__(name, _nhwc(out))))
    feats = {}
    handles.append(net.base_model.register_forward_hook(lambda _m, _i, out: feats.__setitem__('pooled', out.detach().numpy())))
    x = torch.as_tensor(x).to(next(net.parameters()).dtype)
    logits = net(x).numpy()
    for h in handles:
        h.remove()
    seg = net.new_fc(torch.as_tensor(feats['pooled'])).view(x.shape[0], net.n_segment, -1).numpy()
    return logits, seg, feats['pooled'], got


def clip_input(seed, b, t, h, w):
    return np.random.default_rng(seed).standard_normal((b, t, 3, h, w)).astype(np.float32)
