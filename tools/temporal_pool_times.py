"""Launch time of the temporal pool (temporal_maxpool_kernel) inside a temporal-pool TSM-R50 forward at 224^2, T = 8, 32 clips,
in f32 and bf16x3, beside what ``maxpool3x3s2_kernel`` reaches per op on the stem's tensor of the same batch.  DESIGN 4.21.

    python tools/temporal_pool_times.py <out.json> [clips]

The pool has no entry point of its own, so its time is the engine's per-launch timing slot ``layer2.tpool`` (one event before
and one after the launch, inside a whole forward: layer1's output has just been written by the conv before it).  3 warm-up
rounds, then 10 rounds in which the three forms alternate -- a timed forward of the f32 engine, one of the bf16x3 engine, one
``maxpool3x3s2_nhwc`` call on a [clips * 8, 112, 112, 64] fp32 tensor between its own pair of events; the median (and min /
max) is reported.  With X the bytes of layer1's output the pool moves 1.5 X (X in, X / 2 out; both formats store 4 bytes per
element); the spatial pool moves 1.25 of its input.  ``gb_per_s`` is that count over the median.  No figure here is a pass
condition."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                      # noqa: E402

from workoutdetector_amd import _lib                                          # noqa: E402
from workoutdetector_amd.engine import TsmEngine, maxpool3x3s2_nhwc          # noqa: E402
from workoutdetector_amd.weights import make_state_dict                       # noqa: E402

out_path = sys.argv[1]
CLIPS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
T, SIZE, WARM, ROUNDS = 8, 224, 3, 10

sd = make_state_dict(0, 12)
gen = torch.Generator(device='cuda').manual_seed(0)
clips = torch.randn(CLIPS, T, 3, SIZE, SIZE, device='cuda', generator=gen)
engines = {d: TsmEngine(num_class=12, num_segments=T, height=SIZE, width=SIZE, max_clips=CLIPS, state_dict=sd, dtype=d,
                        temporal_pool=True).warmup([CLIPS]) for d in ('f32', 'bf16x3')}
stem = torch.randn(CLIPS * T, 112, 112, 64, device='cuda', generator=gen)
stem_out = torch.empty(CLIPS * T, 56, 56, 64, device='cuda')
logits = torch.empty(CLIPS, 12, device='cuda')


def pool_slot(eng):
    eng.set_layer_timing(1)
    eng.forward_device(clips, out=logits)
    torch.cuda.synchronize()
    return eng.layer_times_ms(0)['layer2.tpool']


def spatial_pool():
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    maxpool3x3s2_nhwc(stem, out=stem_out)
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


forms = {'temporal_maxpool f32': lambda: pool_slot(engines['f32']), 'temporal_maxpool bf16x3': lambda: pool_slot(engines['bf16x3']),
         'maxpool3x3s2 f32 (per op)': spatial_pool}
x_bytes = CLIPS * T * 56 * 56 * 256 * 4
moved = {'temporal_maxpool f32': 1.5 * x_bytes, 'temporal_maxpool bf16x3': 1.5 * x_bytes, 'maxpool3x3s2 f32 (per op)': 1.25 * stem.numel() * 4}
times = {f: [] for f in forms}
for rnd in range(WARM + ROUNDS):
    for f, fn in forms.items():
        t = fn()
        if rnd >= WARM:
            times[f].append(t)
res = {'clips': CLIPS, 'segments': T, 'size': SIZE, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
       'build': _lib.load().tsm_build_id().decode(), 'layer1_output_bytes': x_bytes, 'forms': {}}
for f in forms:
    med = statistics.median(times[f])
    res['forms'][f] = {'ms_median': med, 'ms_min': min(times[f]), 'ms_max': max(times[f]), 'bytes_moved': moved[f],
                       'gb_per_s': moved[f] / (med * 1e-3) / 1e9}
for eng in engines.values():
    eng.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
