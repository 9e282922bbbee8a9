"""Generate tests/golden/ref_tdn.npz by EXECUTING the reference's own TDN classes (build container only), by
make_reference_vectors.py's method: models/tdn.py is read as text at run time, the classes TDN_Net, FBResNet, Bottleneck,
BottleneckShift, mSEModule and ShiftModule are pulled out of it with ``ast`` and executed with torch alone.  The fixture holds
OUTPUTS only (data, no reference text); inputs and weights are the seeded ones of tests/_tdn.py and are not stored:

  mse_out      mSEModule(128, n_segment=3) on x = make_input-style N(0, 1) [6, 128, 5, 6], weights draw_weights(module, 11)
  shift_out    ShiftModule(128, 3) on the same x, weights draw_weights(module, 12)
  logits, features and strided samples of the small taps of one whole TDN_Net: depths (1, 2, 1, 2), T = 3, 2 clips, 96 x 160,
  weights _tdn.build(num_class 7, seed 5), input _tdn.make_input(5, 2, 3, 96, 160); float64, avgpool = AdaptiveAvgPool2d(1) as TSN
  sets it.

Run:  python tests/golden/make_tdn_vectors.py [path of the reference's workoutdetector package]
"""
import ast
import math
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)
import _tdn  # noqa: E402

WANT = ('TDN_Net', 'FBResNet', 'Bottleneck', 'BottleneckShift', 'mSEModule', 'ShiftModule')
NET = dict(num_class=7, T=3, depths=(1, 2, 1, 2), seed=5, clips=2, H=96, W=160)
MODULE_X = dict(seed=21, shape=(6, 128, 5, 6))
TAP_STRIDE = 97      # every 97th element of a tap, flattened NHWC
TAPS = ('diff.stem', 'fuse1', 'fuse2', 'layer2.0.conv1', 'layer2.0.mse.fwd', 'layer2.0.mse.bwd', 'layer2.0.shift', 'layer2.1', 'layer3.0.shift',
        'layer4.1.mse.bwd', 'layer4.1')


def reference_classes(ref_root):
    tree = ast.parse(open(os.path.join(ref_root, 'models', 'tdn.py')).read())
    body = [n for n in tree.body if isinstance(n, ast.ClassDef) and n.name in WANT]
    assert sorted(n.name for n in body) == sorted(WANT)
    ns = dict(torch=torch, nn=nn, F=F, math=math)
    exec(compile(ast.Module(body=body, type_ignores=[]), 'tdn.py', 'exec'), ns)
    return ns


def module_input():
    return torch.from_numpy(np.random.default_rng(MODULE_X['seed']).standard_normal(MODULE_X['shape']))


def main():
    if len(sys.argv) > 1:
        ref_root = sys.argv[1]
    else:
        from make_reference_vectors import REF as ref_root
    ns = reference_classes(ref_root)
    out = {}
    with torch.no_grad():
        mse = ns['mSEModule'](128, n_segment=3).double()
        _tdn.load(mse, _tdn.draw_weights(mse, 11))
        out['mse_out'] = mse(module_input()).numpy()
        shift = ns['ShiftModule'](128, 3).double()
        _tdn.load(shift, _tdn.draw_weights(shift, 12))
        out['shift_out'] = shift(module_input()).numpy()

        T, depths = NET['T'], list(NET['depths'])
        _mine, weights = _tdn.build(NET['num_class'], T, NET['depths'], NET['seed'])
        a, b = (ns['FBResNet'](T, ns['BottleneckShift'], depths, NET['num_class']) for _ in range(2))
        net = ns['TDN_Net'](a, b, 0.75, 0.25)      # tdn_net's rule for T != 8
        net.avgpool = nn.AdaptiveAvgPool2d(1)
        net.fc = nn.Identity()                     # TSN replaces it by Dropout and adds new_fc behind
        net = net.double().eval()
        sd = {k[len('base_model.'):]: torch.from_numpy(v).double() for k, v in weights.items() if k.startswith('base_model.')}
        missing, unexpected = net.load_state_dict(sd, strict=False)
        assert not unexpected and all('num_batches_tracked' in k for k in missing), (missing, unexpected)
        taps = {}

        def hook(name, first=False):      # (a forward hook that returns a value replaces the output: these return None)
            def f(_m, _i, o):
                if not (first and name in taps):
                    taps[name] = _tdn.nhwc(o)
            return f

        def mse_hook(p):                  # m+ / m- are the inputs of the two mse.conv3 calls, forward first
            def f(_m, i, _o):
                taps[p + ('.mse.bwd' if p + '.mse.fwd' in taps else '.mse.fwd')] = _tdn.nhwc(i[0])
            return f

        net.maxpool_diff.register_forward_hook(hook('diff.stem'))
        for li in (2, 3, 4):
            for bi, blk in enumerate(getattr(net, f'layer{li}_bak')):
                p = f'layer{li}.{bi}'
                blk.register_forward_hook(hook(p))
                blk.relu.register_forward_hook(hook(p + '.conv1', first=True))      # (the block's ReLU runs three times: conv1's is the first)
                blk.shift.register_forward_hook(hook(p + '.shift'))
                blk.mse.conv3.register_forward_hook(mse_hook(p))
        net.layer1_bak.register_forward_pre_hook(lambda _m, i: taps.__setitem__('fuse1', _tdn.nhwc(i[0])))
        net.layer2_bak.register_forward_pre_hook(lambda _m, i: taps.__setitem__('fuse2', _tdn.nhwc(i[0])))
        x = torch.from_numpy(_tdn.make_input(NET['seed'], NET['clips'], T, NET['H'], NET['W']))
        feats = net(x)
        w, bias = (torch.from_numpy(weights[k]).double() for k in ('new_fc.weight', 'new_fc.bias'))
        out['features'] = feats.numpy()
        out['logits'] = (feats @ w.t() + bias).view(-1, T, NET['num_class']).mean(1).numpy()
        for name in TAPS:
            out['tap:' + name] = taps[name].reshape(-1)[::TAP_STRIDE].copy()
            out['shape:' + name] = np.array(taps[name].shape)
    np.savez_compressed(os.path.join(HERE, 'ref_tdn.npz'), **out)
    print({k: v.shape for k, v in out.items()})


if __name__ == '__main__':
    main()
