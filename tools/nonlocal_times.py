"""Launch time of ``tsm_nonlocal_attention`` (nonlocal_attn_kernel, fp32, online softmax) at the shapes of the non-local TSM-R50
-- layer2 / layer3 at 224^2, T = 8 and at 256^2, T = 16 -- for 32 clips, beside what torch offers for the same operator in fp32
on the same GPU: ``torch.nn.functional.scaled_dot_product_attention(..., scale=1.0)`` and the ``matmul`` / ``softmax`` /
``matmul`` composite (which materialises the 32 x N_q x N_k scores).  DESIGN 4.19.

    python tools/nonlocal_times.py <out.json> [clips]

Per shape: 3 warm-up rounds, then 10 rounds in which the three forms alternate, each between its own pair of device events; the
median (and min / max) is reported.  ``tflops`` counts the 4 * clips * N_q * N_k * d FLOPs of the two products, and
``peak_frac`` is that rate over the 157.3 TFLOP/s exact-fp32 MFMA peak (MI355X_MICROARCH.md): the kernel's compute-bound share
of peak (its HBM traffic, q + k + v + y once, is far from the bandwidth bound).  A form that cannot run at a shape (out of memory)
is recorded as null with the error's first line.  No ratio here is a pass condition."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch                      # noqa: E402
import torch.nn.functional as F   # noqa: E402

from workoutdetector_amd import _lib                                # noqa: E402
from workoutdetector_amd.engine import nonlocal_attention          # noqa: E402

out_path = sys.argv[1]
CLIPS = int(sys.argv[2]) if len(sys.argv) > 2 else 32
WARM, ROUNDS = 3, 10
PEAK_F32_MFMA_TFLOPS = 157.3
SHAPES = [('224x224 T8 layer2', 6272, 1568, 256), ('224x224 T8 layer3', 1568, 392, 512),
          ('256x256 T16 layer2', 16384, 4096, 256), ('256x256 T16 layer3', 4096, 1024, 512)]


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


res = {'clips': CLIPS, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0), 'build': _lib.load().tsm_build_id().decode(),
       'peak_f32_mfma_tflops': PEAK_F32_MFMA_TFLOPS, 'shapes': {}}
g = torch.Generator(device='cuda').manual_seed(0)
for name, nq, nk, d in SHAPES:
    s = (1.5 / d ** 0.5) ** 0.5                      # scores of standard deviation 1.5: neither uniform nor one-hot
    q = torch.randn(CLIPS, nq, d, device='cuda', generator=g) * s
    k = torch.randn(CLIPS, nk, d, device='cuda', generator=g) * s
    v = torch.randn(CLIPS, nk, d, device='cuda', generator=g)
    ours, kept = torch.empty(CLIPS, nq, d, device='cuda'), {}
    forms = {'nonlocal_attn_kernel': lambda: nonlocal_attention(q, k, v, out=ours),
             'torch_sdpa_scale1': lambda: kept.__setitem__('sdpa', F.scaled_dot_product_attention(q, k, v, scale=1.0)),
             'torch_matmul_softmax_matmul': lambda: kept.__setitem__('mm', torch.softmax(q @ k.transpose(1, 2), dim=-1) @ v)}
    times, errors = {f: [] for f in forms}, {}
    for rnd in range(WARM + ROUNDS):
        for f, fn in forms.items():
            if f in errors:
                continue
            try:
                t = timed(fn)
            except RuntimeError as err:              # (out of memory for the materialised scores)
                errors[f] = str(err).splitlines()[0]
                kept.clear()
                torch.cuda.empty_cache()
                continue
            if rnd >= WARM:
                times[f].append(t)
    flops = 4.0 * CLIPS * nq * nk * d
    row = {'nq': nq, 'nk': nk, 'd': d, 'gflop': flops / 1e9}
    for f in forms:
        if f in errors:
            row[f] = None
            row[f + '_error'] = errors[f]
            continue
        med = statistics.median(times[f])
        row[f] = {'ms_median': med, 'ms_min': min(times[f]), 'ms_max': max(times[f]), 'tflops': flops / (med * 1e-3) / 1e12,
                  'peak_frac': flops / (med * 1e-3) / 1e12 / PEAK_F32_MFMA_TFLOPS}
    for f, key in (('torch_sdpa_scale1', 'sdpa'), ('torch_matmul_softmax_matmul', 'mm')):
        if key in kept:
            row['max_abs_difference_to_' + key] = float((ours - kept[key]).abs().max())
    res['shapes'][name] = row
    del q, k, v, ours, kept
    torch.cuda.empty_cache()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
