"""The float64 reference of the ConvNeXt image model (``TsmEngine(base_model='convnext_base')``), written from the operator's
definition (include/tsm_hip.h, tsm_set_convnext) with timm 0.5.4's key spelling.  Activations are NHWC float64 arrays, the
engine's tap layout.

    stem        Conv2d(3, 128, k 4, s 4, bias) + LayerNorm
    stage s > 0 LayerNorm + Conv2d(C / 2, C, k 2, s 2, bias), floor mode
    block       x + gamma * fc2(GELU(fc1(LN(dwconv7x7(x)))))       (exact GELU, no activation behind the add)
    head        mean over H x W, LayerNorm, fc

Every LayerNorm: over the channels of one pixel, biased variance, eps 1e-6, affine.
"""
import math

import numpy as np

LN_EPS = 1e-6
WIDTHS = (128, 256, 512, 1024)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def layer_norm(x, w, b):
    x = f64(x)
    mean = x.mean(axis=-1, keepdims=True)
    var = ((x - mean) ** 2).mean(axis=-1, keepdims=True)
    return (x - mean) / np.sqrt(var + LN_EPS) * f64(w) + f64(b)


def gelu(x):
    import torch
    x = f64(x)
    return 0.5 * x * (1.0 + torch.erf(torch.from_numpy(np.ascontiguousarray(x / math.sqrt(2.0)))).numpy())


def patch_conv(x, w, b, k):
    """Conv2d(kernel k, stride k, no padding) of NHWC x with OIHW w: the last h % k rows / w % k columns are dropped."""
    x, w = f64(x), f64(w)
    n, h, wd, c = x.shape
    ho, wo = h // k, wd // k
    p = x[:, :ho * k, :wo * k].reshape(n, ho, k, wo, k, c)            # [n, oy, ky, ox, kx, c]
    return np.einsum('nyaxbc,ocab->nyxo', p, w) + f64(b)


def dwconv7(x, w, b):
    """Depthwise 7x7, padding 3, of NHWC x with w [C, 1, 7, 7]."""
    x, w = f64(x), f64(w)
    n, h, wd, c = x.shape
    xp = np.zeros((n, h + 6, wd + 6, c))
    xp[:, 3:3 + h, 3:3 + wd] = x
    out = np.zeros_like(x) + f64(b)
    for ky in range(7):
        for kx in range(7):
            out += xp[:, ky:ky + h, kx:kx + wd] * w[:, 0, ky, kx]
    return out


def linear(x, w, b):
    return f64(x) @ f64(w).T + f64(b)


def block_parts(sd, p, x):
    """{'.dwln', '.fc1' (behind the GELU), '' (the block's output)} of block ``p`` = 'stages.S.blocks.B' on input x."""
    dwln = layer_norm(dwconv7(x, sd[p + '.conv_dw.weight'], sd[p + '.conv_dw.bias']), sd[p + '.norm.weight'], sd[p + '.norm.bias'])
    fc1 = gelu(linear(dwln, sd[p + '.mlp.fc1.weight'], sd[p + '.mlp.fc1.bias']))
    out = f64(x) + f64(sd[p + '.gamma']) * linear(fc1, sd[p + '.mlp.fc2.weight'], sd[p + '.mlp.fc2.bias'])
    return {'.dwln': dwln, '.fc1': fc1, '': out}


def stem(sd, x_nchw):
    x = f64(x_nchw).transpose(0, 2, 3, 1)
    return layer_norm(patch_conv(x, sd['stem.0.weight'], sd['stem.0.bias'], 4), sd['stem.1.weight'], sd['stem.1.bias'])


def downsample(sd, s, x):
    p = f'stages.{s}.downsample'
    return patch_conv(layer_norm(x, sd[p + '.0.weight'], sd[p + '.0.bias']), sd[p + '.1.weight'], sd[p + '.1.bias'], 2)


def head_norm(sd, x):
    pool = f64(x).mean(axis=(1, 2))
    return pool, layer_norm(pool, sd['head.norm.weight'], sd['head.norm.bias'])


def forward(sd, x_nchw, depths, keep=()):
    """The whole model on x [n, 3, H, W]: {'logits', 'head.pool', 'head.norm', 'stem'} plus every tap named in ``keep``
    ('stages.S.downsample', 'stages.S.blocks.B', '....dwln', '....fc1') and 'rms': the root mean square of every block's output."""
    out, rms = {}, []
    x = out['stem'] = stem(sd, x_nchw)
    for s, nb in enumerate(depths):
        if s > 0:
            x = downsample(sd, s, x)
            if f'stages.{s}.downsample' in keep:
                out[f'stages.{s}.downsample'] = x
        for b in range(nb):
            p = f'stages.{s}.blocks.{b}'
            parts = block_parts(sd, p, x)
            for part, v in parts.items():
                if p + part in keep:
                    out[p + part] = v
            x = parts['']
            rms.append(float(np.sqrt((x ** 2).mean())))
    pool, norm = head_norm(sd, x)
    out.update({'head.pool': pool, 'head.norm': norm, 'logits': linear(norm, sd['head.fc.weight'], sd['head.fc.bias']), 'rms': rms})
    return out
