"""TDN-ResNet50 as a torch module tree with the TSN module's key names, written from the definition in include/tsm_hip.h
(tsm_set_tdn), and the seeded weight recipe of the TDN tests.  tests/test_tdn_cpu.py pins this model to the reference through
tests/golden/ref_tdn.npz; the GPU tests then need neither the reference nor the fixture's source.

    model = TDN(num_class, T, depths).double(); load(model, draw_weights(model, seed))
    logits, taps = model(x, taps=True)          # x [n_clips * T, 15, H, W]; taps are NHWC, under the engine's tap names

build(..., recipe=f) applies a state-dict transform behind the draw (residual_gain, small_variance, gate_gain: the crafted networks
of tests/_tdn_cases.py); its defaults are the fixture's network.
"""
from __future__ import annotations

import re
from collections import OrderedDict

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

PLANES = (64, 128, 256, 512)


def nearest_index(dst: int, n_in: int, n_out: int) -> int:
    """torch's 'nearest': min(int(floorf(dst * ((float)in / out))), in - 1), in float32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return min(int(np.floor(np.float32(dst) * scale)), n_in - 1)


def up(x: torch.Tensor, size) -> torch.Tensor:
    """Nearest upsample of [N, C, h, w] to ``size`` by the index formula (not F.interpolate: the CPU test compares the two)."""
    iy = torch.tensor([nearest_index(i, x.shape[2], size[0]) for i in range(size[0])])
    ix = torch.tensor([nearest_index(i, x.shape[3], size[1]) for i in range(size[1])])
    return x[:, :, iy][:, :, :, ix]


def conv_bn(cin, cout, k, stride=1, bias=True):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=k // 2, bias=bias), nn.BatchNorm2d(cout)


class MSE(nn.Module):
    """The long-term module's gate: x [N, C, H, W] -> g = x + x y.  ``gate`` / ``swap_ends`` are the CPU test's ablations."""

    def __init__(self, c: int, n_segment: int):
        super().__init__()
        r = c // 16
        self.n_segment, self.gate, self.swap_ends = n_segment, True, False
        self.conv1, self.bn1 = conv_bn(c, r, 1, bias=False)
        self.conv2 = nn.Conv2d(r, r, 3, padding=1, groups=r, bias=False)
        self.conv3, self.bn3 = conv_bn(r, c, 1, bias=False)
        self.conv3_smallscale2, self.bn3_smallscale2 = conv_bn(r, r, 3, bias=False)
        self.conv3_smallscale4, self.bn3_smallscale4 = conv_bn(r, r, 3, bias=False)

    def directions(self, x):
        """m+, m- [N, r, H, W] and e+, e- [N, C, H, W]."""
        T = self.n_segment
        b = self.bn1(self.conv1(x))
        c = self.conv2(b)
        bt, ct = b.view((-1, T) + b.shape[1:]), c.view((-1, T) + c.shape[1:])
        zero = torch.zeros_like(bt[:, :1])
        fwd, bwd = ct[:, 1:] - bt[:, :-1], ct[:, :-1] - bt[:, 1:]
        d_f = torch.cat([fwd, zero] if not self.swap_ends else [zero, fwd], 1).reshape(b.shape)      # 0 at t = T - 1
        d_b = torch.cat([zero, bwd] if not self.swap_ends else [bwd, zero], 1).reshape(b.shape)      # 0 at t = 0
        ms, es = [], []
        for d in (d_f, d_b):
            s2 = self.bn3_smallscale2(self.conv3_smallscale2(F.avg_pool2d(d, 2, 2)))
            s4 = self.bn3_smallscale4(self.conv3_smallscale4(d))
            m = d / 3 + up(s2, d.shape[2:]) / 3 + s4 / 3
            ms.append(m)
            es.append(self.bn3(self.conv3(m)))
        return ms, es

    def forward(self, x, taps=None, name=''):
        ms, es = self.directions(x)
        if taps is not None:
            taps[name + '.mse.fwd'], taps[name + '.mse.bwd'] = nhwc(ms[0]), nhwc(ms[1])
            taps[name + '.mse.e'] = torch.cat(es).detach()
        if not self.gate:
            return x
        y = 0.5 * (torch.sigmoid(es[0]) - 0.5) + 0.5 * (torch.sigmoid(es[1]) - 0.5)
        return x + x * y


class Shift(nn.Module):
    """o[t, c] = w[c, 0] g[t - 1, c] + w[c, 1] g[t, c] + w[c, 2] g[t + 1, c] per clip, zeros beyond its ends."""

    def __init__(self, c: int, n_segment: int):
        super().__init__()
        self.n_segment = n_segment
        self.conv = nn.Conv1d(c, c, 3, padding=1, groups=c, bias=False)

    def forward(self, g):
        T = self.n_segment
        gt = g.view((-1, T) + g.shape[1:])
        z = torch.zeros_like(gt[:, :1])
        w = self.conv.weight[:, 0].view(1, 1, -1, 1, 1, 3)
        prev, nxt = torch.cat([z, gt[:, :-1]], 1), torch.cat([gt[:, 1:], z], 1)
        return (w[..., 0] * prev + w[..., 1] * gt + w[..., 2] * nxt).reshape(g.shape)


class Block(nn.Module):
    def __init__(self, cin: int, planes: int, stride: int, down: bool, n_segment: int, long_term: bool):
        super().__init__()
        self.conv1, self.bn1 = conv_bn(cin, planes, 1)
        if long_term:
            self.mse, self.shift = MSE(planes, n_segment), Shift(planes, n_segment)
        self.conv2, self.bn2 = conv_bn(planes, planes, 3, stride)
        self.conv3, self.bn3 = conv_bn(planes, 4 * planes, 1)
        self.downsample = nn.Sequential(*conv_bn(cin, 4 * planes, 1, stride)) if down else None

    def forward(self, x, taps=None, name=''):
        out = F.relu(self.bn1(self.conv1(x)))
        if taps is not None:
            taps[name + '.conv1'] = nhwc(out)
        if hasattr(self, 'mse'):
            out = self.shift(self.mse(out, taps, name))
            if taps is not None:
                taps[name + '.shift'] = nhwc(out)
        out = F.relu(self.bn2(self.conv2(out)))
        if taps is not None:
            taps[name + '.conv2'] = nhwc(out)
        out = F.relu(self.bn3(self.conv3(out)) + (x if self.downsample is None else self.downsample(x)))
        if taps is not None:
            taps[name] = nhwc(out)
        return out


def stage(cin, planes, blocks, stride, n_segment, long_term):
    return nn.Sequential(*[Block(cin if b == 0 else 4 * planes, planes, stride if b == 0 else 1, b == 0, n_segment, long_term)
                           for b in range(blocks)])


class Base(nn.Module):
    def __init__(self, n_segment: int, depths, alpha: float, beta: float):
        super().__init__()
        self.alpha, self.beta = alpha, beta
        self.conv1, self.bn1 = conv_bn(3, 64, 7, 2)
        self.conv1_temp = nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=True)      # in every checkpoint, unused by the forward
        self.conv1_5 = nn.Sequential(*conv_bn(12, 64, 7, 2, bias=False), nn.ReLU())
        self.resnext_layer1 = stage(64, 64, depths[0], 1, n_segment, False)
        self.layer1_bak = stage(64, 64, depths[0], 1, n_segment, False)
        self.layer2_bak = stage(256, 128, depths[1], 2, n_segment, True)
        self.layer3_bak = stage(512, 256, depths[2], 2, n_segment, True)
        self.layer4_bak = stage(1024, 512, depths[3], 2, n_segment, True)

    def forward(self, x, taps=None):
        def note(name, t):
            if taps is not None:
                taps[name] = nhwc(t)

        def run(layer, name, t):
            for b, blk in enumerate(layer):
                t = blk(t, taps, f'{name}.{b}')
            return t

        f = [x[:, 3 * i:3 * i + 3] for i in range(5)]
        d = torch.cat([f[i + 1] - f[i] for i in range(4)], 1)
        xc5 = self.conv1_5(F.avg_pool2d(d, 2, 2))
        note('diff.conv1_5', xc5)
        xd0 = F.max_pool2d(xc5, 3, 2, 1)
        note('diff.stem', xd0)
        xd1 = run(self.resnext_layer1, 'resnext_layer1', xd0)
        s = F.max_pool2d(F.relu(self.bn1(self.conv1(f[2]))), 3, 2, 1)
        note('stem', s)
        t = self.alpha * s + self.beta * up(xd0, s.shape[2:])
        note('fuse1', t)
        t = run(self.layer1_bak, 'layer1', t)
        t = self.alpha * t + self.beta * up(xd1, t.shape[2:])
        note('fuse2', t)
        for li in (2, 3, 4):
            t = run(getattr(self, f'layer{li}_bak'), f'layer{li}', t)
        return t.mean((2, 3))


class TDN(nn.Module):
    """x [n_clips * T, 15, H, W] -> logits [n_clips, num_class] ('avg') or [n_clips, T, num_class] ('identity')."""

    def __init__(self, num_class: int, n_segment: int, depths=(3, 4, 6, 3), alpha=None, beta=None, consensus: str = 'avg'):
        super().__init__()
        if alpha is None:
            alpha, beta = (0.5, 0.5) if n_segment == 8 else (0.75, 0.25)
        self.n_segment, self.consensus = n_segment, consensus
        self.base_model = Base(n_segment, depths, alpha, beta)
        self.new_fc = nn.Linear(2048, num_class)

    def forward(self, x, taps: bool = False):
        t = OrderedDict() if taps else None
        feats = self.base_model(x, t)
        out = self.new_fc(feats).view(-1, self.n_segment, self.new_fc.out_features)
        out = out.mean(1) if self.consensus == 'avg' else out
        if taps:
            t['features'] = feats.detach().numpy()
            return out, t
        return out


def nhwc(t: torch.Tensor) -> np.ndarray:
    return t.detach().permute(0, 2, 3, 1).contiguous().numpy()


def draw_weights(module: nn.Module, seed: int) -> 'OrderedDict[str, np.ndarray]':
    """The tests' seeded recipe, drawn with np.random.default_rng(seed) in sorted key order (float64): conv weights
    N(0, sqrt(2 / (k^2 cout))), conv biases N(0, 0.1), BatchNorm weight and variance U(0.5, 1.5), bias and mean N(0, 0.1), temporal
    weights N(0, 0.5), the classifier N(0, 0.05) / N(0, 0.1)."""
    rng = np.random.default_rng(seed)
    sd = module.state_dict()
    out = {}
    for key in sorted(sd):
        shape = tuple(sd[key].shape)
        if key.endswith('num_batches_tracked'):
            continue
        if key.endswith('running_var') or (key.endswith('.weight') and len(shape) == 1):
            a = rng.uniform(0.5, 1.5, shape)
        elif len(shape) == 4:
            a = rng.standard_normal(shape) * np.sqrt(2.0 / (shape[2] * shape[3] * shape[0]))
        elif len(shape) == 3:
            a = rng.standard_normal(shape) * 0.5
        elif len(shape) == 2:
            a = rng.standard_normal(shape) * 0.05
        else:
            a = rng.standard_normal(shape) * 0.1
        out[key] = a
    return OrderedDict((k, out[k]) for k in sd if k in out)


def load(module: nn.Module, weights) -> nn.Module:
    module.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in weights.items()}, strict=False)
    return module.eval()


def make_input(seed: int, n_clips: int, T: int, H: int, W: int) -> np.ndarray:
    """[n_clips * T, 15, H, W] float64, N(0, 1)."""
    return np.random.default_rng([seed, n_clips, T, H, W]).standard_normal((n_clips * T, 15, H, W))


def build(num_class: int, T: int, depths, seed: int, consensus: str = 'avg', dtype=torch.float64, recipe=None):
    """The seeded model in ``dtype`` and its weights as float32 arrays (what an engine loads).  ``recipe``: a function of the
    float32 weights that returns the float32 weights to use (residual_gain, small_variance, gate_gain below, or a composition)."""
    model = TDN(num_class, T, depths, consensus=consensus).to(dtype)
    w = OrderedDict((k, np.asarray(v, dtype=np.float32)) for k, v in draw_weights(model, seed).items())
    if recipe is not None:
        w = recipe(w)
        assert all(v.dtype == np.float32 for v in w.values())
    load(model, w)      # the model computes in `dtype` FROM the fp32 weights
    return model, w


# ---- recipes: state-dict transforms behind draw_weights, float32 in and float32 out ---------------------------------------------
def _times(w, pattern: str, k: float):
    out = OrderedDict(w)
    hit = [key for key in w if re.search(pattern, key)]
    assert hit, pattern
    for key in hit:
        out[key] = w[key] * np.float32(k)
    return out


def residual_gain(w, g: float):
    """Every Block.bn3.weight (the residual branch's last BatchNorm, both paths; not the mSE's bn3) times g."""
    return _times(w, r'\.\d+\.bn3\.weight$', g)


def gate_gain(w, k: float):
    """Every mse.bn3.weight and mse.bn3.bias times k: the gates' pre-activations e times k."""
    return _times(w, r'\.mse\.bn3\.(weight|bias)$', k)


def small_variance(w, seed: int):
    """Every BatchNorm's running_var log-uniform in [1e-6, 1e-4] (np.random.default_rng(seed), sorted key order), as float32, and
    its weight times sqrt(var + 1e-5) in float32: the folded scale keeps the size it had, and eps = 1e-5 is a tenth to ten times
    the variance under the root."""
    rng = np.random.default_rng(seed)
    out = OrderedDict(w)
    for key in sorted(w):
        if not key.endswith('running_var'):
            continue
        var = np.exp(rng.uniform(np.log(1e-6), np.log(1e-4), w[key].shape)).astype(np.float32)
        gamma = key[:-len('running_var')] + 'weight'
        out[key] = var
        out[gamma] = w[gamma] * np.sqrt(var + np.float32(1e-5))
        assert out[gamma].dtype == np.float32
    return out


def set_eps(model: nn.Module, eps: float, only_mse: bool = False) -> nn.Module:
    """The eps of every BatchNorm of ``model`` (only_mse: of the four inside every MSE) -- the CPU tests' mutation."""
    roots = [m for m in model.modules() if isinstance(m, MSE)] if only_mse else [model]
    n = 0
    for root in roots:
        for m in root.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eps = eps
                n += 1
    assert n > 0
    return model
