"""Head-slot time and clips/s of avg / identity engines (TSM-R50, T = 8, 224x224, seed-0 weights, tuned), the engines
alternating in ONE process: median of 20 steps of ``last_forward_ms`` (clips/s), then 20 steps under per-launch timing
(``layer_times_ms()['head']``).  DESIGN 4.13.

    python tools/head_times.py <tree> <dtype> <consensus[,consensus]> <out.json> [clips]

``<tree>`` is the checkout whose package and library are measured: ``.`` for this one, or a checkout of another commit with
its library built (an older one knows 'avg' only)."""
import json
import os
import statistics
import sys

root, dtype, kinds, out_path = sys.argv[1], sys.argv[2], sys.argv[3].split(','), sys.argv[4]
B = int(sys.argv[5]) if len(sys.argv) > 5 else int(os.environ.get('MEASURE_B', '32'))
sys.path.insert(0, os.path.abspath(root))
os.environ.setdefault('TSM_TUNE_CACHE', 'off')

import numpy as np      # noqa: E402
import torch            # noqa: E402

from workoutdetector_amd.engine import TsmEngine              # noqa: E402
from workoutdetector_amd.weights import make_state_dict       # noqa: E402

T, S, STEPS = 8, 224, 20
sd = make_state_dict(0, 12)
x = torch.from_numpy(np.random.default_rng(0).standard_normal((B, T, 3, S, S)).astype(np.float32)).cuda()
engines = {}
for k in kinds:
    kw = {} if k == 'avg' else {'consensus_type': k}
    engines[k] = TsmEngine(num_class=12, num_segments=T, height=S, width=S, max_clips=B, state_dict=sd, dtype=dtype, **kw)
    engines[k].warmup([B])
for _ in range(5):
    for e in engines.values():
        e.forward_device(x)
torch.cuda.synchronize()
fwd = {k: [] for k in kinds}
for _ in range(STEPS):
    for k, e in engines.items():
        e.forward_device(x)
        torch.cuda.synchronize()
        fwd[k].append(e.last_forward_ms)
for e in engines.values():
    e.set_layer_timing(STEPS)
for _ in range(STEPS):
    for e in engines.values():
        e.forward_device(x)
        torch.cuda.synchronize()
res = {'tree': root, 'dtype': dtype, 'B': B}
for k, e in engines.items():
    head = [e.layer_times_ms(i)['head'] for i in range(STEPS)]
    m = statistics.median(fwd[k])
    res[k] = {'forward_ms_median': m, 'clips_per_s': B / (m / 1000.0), 'head_ms_median': statistics.median(head),
              'head_ms_min': min(head), 'head_ms_max': max(head)}
    e.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f)
