"""Per-launch times of the non-local R50 (f32, 32 clips, 224^2, T = 8): which launch dominates the time the blocks add.

    python tools/nonlocal_layer_times.py [out.json]

The bucket is tuned first (never timed), 3 untimed forwards, then 5 forwards with per-launch events (tsm_set_layer_timing);
medians per launch, summed per part (theta | phi | g conv, pool, attention, W conv).  DESIGN 4.19."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from workoutdetector_amd.engine import create_model
b = 32
eng = create_model(num_class=12, non_local=True, max_clips=b)
x = torch.randn(b, 8, 3, 224, 224, device='cuda')
eng.warmup([b])
for _ in range(3):
    eng.forward_device(x)
torch.cuda.synchronize()
eng.set_layer_timing(5)
for _ in range(5):
    eng.forward_device(x)
torch.cuda.synchronize()
rows = [eng.layer_times_ms(i) for i in range(5)]
med = {k: statistics.median(r[k] for r in rows) for k in rows[0]}
nl = {k: v for k, v in med.items() if '.nl.' in k}
parts = {p: sum(v for k, v in nl.items() if k.endswith('.nl.' + p)) for p in ('qkv', 'pool', 'attn', 'W')}
out = {'batch': b, 'total_ms': sum(v for v in med.values() if v > 0), 'nl_ms': sum(nl.values()), 'nl_parts_ms': parts, 'nl_launches_ms': nl,
       'tiles': {k: v for k, v in eng.conv_tiles(b).items() if '.nl.' in k}}
print(json.dumps(out))
if len(sys.argv) > 1:
    with open(sys.argv[1], 'w') as f:
        json.dump(out, f, indent=1)
