"""Times of the ConvNeXt-Base image engine (``create_image_model(base_model='convnext_base')``) at 32 frames of 224 x 224 on one
GPU.  DESIGN 4.24.

    python tools/convnext_times.py <out.json> [frames]

In one process, 3 warm-up rounds, then 10 rounds in which these alternate:
  * a plain forward (``forward_device``) between two device events: frames/s of the whole forward;
  * a forward with per-launch timing (``set_layer_timing``: one device event before and one after every launch, so each figure
    carries the event pair's own cost, a few microseconds): the per-launch medians, summed per kernel family and listed for the
    first block of every stage;
  * per stage, torch's ``conv2d(groups=C)`` + ``layer_norm`` in fp32 on the tensor the stage's first ``dwconv7_ln_kernel``
    launch reads (the engine's own tap, channels-last) with the same weights, between two device events.
Per stage the ``dwconv7_ln_kernel`` launch stands beside its byte bound -- input once, output once, n * H * W * C * 4 bytes
each, over the 8.0 TB/s HBM peak of MI355X_MICROARCH.md (6.3 TB/s is what a copy achieves there) -- and beside torch's time.
No figure here is a pass condition."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np                # noqa: E402
import torch                      # noqa: E402
import torch.nn.functional as F   # noqa: E402

from workoutdetector_amd import _lib, flops                                   # noqa: E402
from workoutdetector_amd.engine import create_image_model                     # noqa: E402
from workoutdetector_amd.weights import CONVNEXT_WIDTHS, make_state_dict      # noqa: E402

out_path = sys.argv[1]
FRAMES = int(sys.argv[2]) if len(sys.argv) > 2 else 32
SIZE, WARM, ROUNDS = 224, 3, 10
HBM_PEAK = 8.0e12


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(v):
    return {'ms_median': statistics.median(v), 'ms_min': min(v), 'ms_max': max(v)}


sd = make_state_dict(0, 2, 'convnext_base')
eng = create_image_model(num_class=2, base_model='convnext_base', max_frames=FRAMES, resize=SIZE, crop=SIZE)
x_host = np.random.default_rng(0).standard_normal((FRAMES, 1, 3, SIZE, SIZE)).astype(np.float32)
x = torch.from_numpy(x_host).cuda()
out = torch.empty(FRAMES, 2, device='cuda')
eng.warmup([FRAMES])

# torch's operands: the engine's own tap in front of every stage's first block, and that block's weights
torch_ops, taps = {}, {}
for s, c in enumerate(CONVNEXT_WIDTHS):
    blk = f'stages.{s}.blocks.0'
    src = eng.forward_tap(x_host, 'stem' if s == 0 else f'stages.{s}.downsample')                   # NHWC
    xin = torch.from_numpy(src).cuda().permute(0, 3, 1, 2)                                           # NCHW view, channels-last memory
    w, b, lw, lb = (torch.from_numpy(sd[blk + k]).cuda() for k in ('.conv_dw.weight', '.conv_dw.bias', '.norm.weight', '.norm.bias'))
    torch_ops[s] = (lambda xin=xin, w=w, b=b, lw=lw, lb=lb, c=c: F.layer_norm(F.conv2d(xin, w, b, padding=3, groups=c).permute(0, 2, 3, 1),
                                                                              (c,), lw, lb, 1e-6))
    taps[s] = (torch.from_numpy(eng.forward_tap(x_host, blk + '.dwln')).cuda(), tuple(src.shape))

names = eng.launch_names()
forward_ms, torch_ms, launch_ms = [], {s: [] for s in torch_ops}, {k: [] for k in names}
for rnd in range(WARM + ROUNDS):
    eng.set_layer_timing(0)
    t_fwd = timed(lambda: eng.forward_device(x, out=out))
    eng.set_layer_timing(1)                              # arms the next forward only
    eng.forward_device(x, out=out)
    t_launch = eng.layer_times_ms(0)                     # (synchronises on the last event)
    t_torch = {s: timed(fn) for s, fn in torch_ops.items()}
    if rnd >= WARM:
        forward_ms.append(t_fwd)
        for k, t in t_launch.items():
            launch_ms[k].append(t)
        for s, t in t_torch.items():
            torch_ms[s].append(t)
eng.set_layer_timing(0)

median = {k: statistics.median(v) for k, v in launch_ms.items()}
families = {}
for k, v in median.items():
    fam = ('dwconv7_ln' if k.endswith('.dwln') else 'fc1' if k.endswith('.fc1') else 'gelu' if k.endswith('.gelu') else 'fc2' if k.endswith('.fc2')
           else 'downsample_ln' if k.endswith('.downsample.norm') else 'downsample' if k.endswith('.downsample') else k)
    if v >= 0:
        families[fam] = families.get(fam, 0.0) + v
res = {'frames': FRAMES, 'size': SIZE, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0), 'build': _lib.load().tsm_build_id().decode(),
       'hbm_peak_bytes_per_s': HBM_PEAK, 'gmac_per_frame': flops.macs_per_frame(SIZE, SIZE, 2, 'convnext_base') / 1e9,
       'forward': dict(stats(forward_ms), frames_per_s=FRAMES / (statistics.median(forward_ms) * 1e-3),
                       tflops=2.0 * flops.macs_per_frame(SIZE, SIZE, 2, 'convnext_base') * FRAMES / (statistics.median(forward_ms) * 1e-3) / 1e12),
       'launches': len(names), 'sum_of_launch_medians_ms': sum(v for v in median.values() if v >= 0),
       'family_ms': families, 'conv_tiles': eng.conv_tiles(FRAMES), 'dwconv7_ln': {}, 'first_block_ms': {}}
for s, c in enumerate(CONVNEXT_WIDTHS):
    blk = f'stages.{s}.blocks.0'
    want, shape = taps[s]
    n, h, w_, _c = shape
    nbytes = 2.0 * n * h * w_ * c * 4
    ours = stats(launch_ms[blk + '.dwln'])
    bound_ms = nbytes / HBM_PEAK * 1e3
    res['dwconv7_ln'][f'C{c} {h}x{w_}'] = {
        'bytes_in_plus_out': nbytes, 'byte_bound_ms': bound_ms, 'dwconv7_ln_kernel': ours, 'bound_over_kernel': bound_ms / ours['ms_median'],
        'achieved_bytes_per_s': nbytes / (ours['ms_median'] * 1e-3), 'torch_conv2d_groups_plus_layer_norm': stats(torch_ms[s]),
        'torch_over_kernel': statistics.median(torch_ms[s]) / ours['ms_median'],
        'max_abs_difference_to_torch': float((torch_ops[s]() - want).abs().max())}
    res['first_block_ms'][blk] = {part: median[blk + '.' + part] for part in ('dwln', 'fc1', 'gelu', 'fc2')}
eng.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
