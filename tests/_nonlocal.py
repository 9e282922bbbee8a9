"""Shared pieces of the non-local tests (tests/test_nonlocal_cpu.py, tests/test_nonlocal_gpu.py).

* ``NonLocal3d`` / ``NLWrapper``: the embedded-Gaussian non-local block and its wrapper with the module tree of the TSM code
  base's NONLocalBlock3D / NL3DWrapper (``block``, ``nl.theta``, ``nl.phi.0``, ``nl.g.0``, ``nl.W.0``, ``nl.W.1``), written from
  the operator's definition (include/tsm_hip.h, tsm_set_non_local).
* ``torch_tsm_nl``: ``tests._torch_tsm.TorchTSM`` with blocks ``NL_BLOCKS`` wrapped afterwards, the way make_non_local does it.
* ``attention_ref``: the bare attention in float64.
* ``run_with_taps``: one forward with forward hooks that record the engine's tap points as NHWC arrays, and per non-local block
  the largest probability of every softmax row.
"""
import numpy as np
import torch
import torch.nn as nn

from tests._torch_tsm import TorchTSM
from workoutdetector_amd.weights import NL_BLOCKS, WIDTHS

TAPS = ('layer2.0', 'layer2.0.block', 'layer2.2.nl.y', 'layer3.4')


class NonLocal3d(nn.Module):
    def __init__(self, c):
        super().__init__()
        d = c // 2
        self.theta = nn.Conv3d(c, d, 1)
        self.phi = nn.Sequential(nn.Conv3d(c, d, 1), nn.MaxPool3d(kernel_size=(1, 2, 2)))
        self.g = nn.Sequential(nn.Conv3d(c, d, 1), nn.MaxPool3d(kernel_size=(1, 2, 2)))
        self.W = nn.Sequential(nn.Conv3d(d, c, 1), nn.BatchNorm3d(c))
        self.row_max, self.n_keys = None, 0

    def forward(self, x):                                  # [B, C, T, H, W]
        b = x.shape[0]
        theta = self.theta(x).flatten(2).transpose(1, 2)   # [B, Nq, d], positions in (t, h, w) order
        phi = self.phi(x).flatten(2)                       # [B, d, Nk]
        g = self.g(x).flatten(2).transpose(1, 2)           # [B, Nk, d]
        p = torch.softmax(theta @ phi, dim=-1)             # no scale factor
        self.row_max, self.n_keys = p.max(dim=-1).values.detach(), p.shape[-1]
        y = (p @ g).transpose(1, 2).reshape(b, -1, *x.shape[2:])
        return self.W(y) + x                               # no ReLU


class NLWrapper(nn.Module):
    def __init__(self, block, n_segment):
        super().__init__()
        self.block = block
        self.nl = NonLocal3d(getattr(block, 'net', block).bn3.num_features)
        self.n_segment = n_segment

    def forward(self, x):
        x = self.block(x)
        nt, c, h, w = x.shape
        x = x.view(nt // self.n_segment, self.n_segment, c, h, w).transpose(1, 2)
        x = self.nl(x)
        return x.transpose(1, 2).reshape(nt, c, h, w)


def torch_tsm_nl(base_model='resnet50', shift_place='blockres', num_class=12, n_segment=8, is_shift=True, sd=None,
                 dtype=torch.float64):
    """TorchTSM with the five blocks wrapped; ``sd`` (engine keys) loaded strictly; eval mode, ``dtype``.  ``is_shift=False``:
    the shift modules stay in the tree (same keys) with a fold of zero channels."""
    net = TorchTSM(base_model, WIDTHS.get(base_model, 64), shift_place, num_class, n_segment, fold_div=8 if is_shift else 1 << 20)
    for li, b in NL_BLOCKS:
        layer = getattr(net.base_model, f'layer{li}')
        layer[b] = NLWrapper(layer[b], n_segment)
    if sd is not None:
        net.load_engine_state_dict(sd)
    return net.to(dtype).eval()


def attention_ref(q, k, v):
    """softmax_j(q . k^T) v in float64: q [B, Nq, d], k / v [B, Nk, d] (any float tensors, any device) -> float64 CPU."""
    q, k, v = (t.detach().to('cpu', torch.float64) for t in (q, k, v))
    return torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v


def _nhwc(t):
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


@torch.no_grad()
def run_with_taps(net, x, taps=TAPS):
    """One forward of ``x`` [B, T, 3, H, W] through ``net`` (its dtype) -> (logits [B, num_class], per-segment logits
    [B, T, num_class], pooled features [B * T, feat], {tap: NHWC ndarray}, {block: (row maxima [B, Nq], Nk)})."""
    got, handles = {}, []
    for name in taps:
        layer, b, *rest = name.split('.')
        mod = getattr(net.base_model, layer)[int(b)]
        if rest == ['block']:
            handles.append(mod.block.register_forward_hook(lambda _m, _i, out, name=name: got.__setitem__(name, _nhwc(out))))
        elif rest == ['nl', 'y']:            # y is W's input [B, d, T, H, W] -> [B * T, H, W, d]
            def pre(_m, inp, name=name):
                y = inp[0].detach()
                got[name] = y.permute(0, 2, 3, 4, 1).reshape(-1, y.shape[3], y.shape[4], y.shape[1]).contiguous().numpy()
            handles.append(mod.nl.W.register_forward_pre_hook(pre))
        else:
            handles.append(mod.register_forward_hook(lambda _m, _i, out, name=name: got.__setitem__(name, _nhwc(out))))
    feats = {}
    handles.append(net.base_model.register_forward_hook(lambda _m, _i, out: feats.__setitem__('pooled', out.detach().numpy())))
    x = torch.as_tensor(x).to(next(net.parameters()).dtype)
    logits = net(x).numpy()
    for h in handles:
        h.remove()
    seg = net.new_fc(torch.as_tensor(feats['pooled'])).view(x.shape[0], net.n_segment, -1).numpy()
    sharp = {f'layer{li}.{b}': (getattr(net.base_model, f'layer{li}')[b].nl.row_max.numpy(),
                                getattr(net.base_model, f'layer{li}')[b].nl.n_keys) for li, b in NL_BLOCKS}
    return logits, seg, feats['pooled'], got, sharp


def clip_input(seed, b, t, h, w):
    return np.random.default_rng(seed).standard_normal((b, t, 3, h, w)).astype(np.float32)
