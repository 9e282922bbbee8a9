"""Clip throughput of the TSM backbones (R18 / R34 / R50 / WRN-50-2) side by side on one GPU: one JSON line per (backbone, dtype).

    python tools/backbone_bench.py [--backbones resnet18,resnet34,resnet50,wide_resnet50_2] [--dtypes f32,bf16] [--batch 32]
                                   [--segments 8] [--size 224] [--steps 20] [--warmup 5] [--shift-place blockres,block]
                                   [--non-local] [--temporal-pool]

One line per (backbone, dtype, shift placement).  Each engine gets the seeded synthetic weights of its backbone
(weights.make_state_dict(0, 12, base_model, shift_place); the same numbers under both placements) and one
device-resident seeded batch [B, T, 3, S, S]; ``warmup()`` tunes the batch's bucket first (never timed), then W untimed
and K timed forwards run back to back on torch's current stream, one event per step boundary.  Fields:

  ms_per_step      median of the K per-step event durations
  clips_per_s      batch / ms_per_step
  gflop_per_step   algorithmic forward work (workoutdetector_amd.flops, 2 FLOPs per MAC; shift / BN / pooling count 0)
  peak_frac        achieved FLOP/s over the exact-fp32 MFMA peak (f32) or the dense bf16 MFMA peak (bf16, bf16x3): a
                   whole-forward figure, not a kernel's share of peak
  logits_err       max |logits - CPU restatement| / max |CPU restatement| on the first two clips of the last timed step:
                   fp32 reference for f32 / bf16x3, the bf16-storage restatement for bf16 (oracle/tsm_oracle.py: one
                   ``forward`` for every backbone and placement)

``--non-local``: every f32 Bottleneck line (resnet50, wide_resnet50_2) is followed by the same engine with
``non_local=True`` (``"non_local": true``; its reference is the float64 torch model of tests/_nonlocal.py), so the plain and the
non-local clips/s stand side by side; every other (backbone, dtype) has no non-local form and prints its plain line only.

``--temporal-pool``: every f32 / bf16x3 line is followed by the same engine with ``temporal_pool=True`` (``"temporal_pool":
true``; its reference is the float64 torch model of tests/_temporal_pool.py, and its FLOPs count layers 2-4 at half the frames), so
the plain and the pooled clips/s of one build stand side by side; bf16 has no pooled form and prints its plain line only.

No CPU fallback: without a GPU it fails.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

PEAK_F32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md, "Peak FP32 (matrix)"
PEAK_BF16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md, "Peak BF16/FP16 MFMA", dense


def reference_logits(base_model, sd, clips, t, dtype, shift_place='blockres', non_local=False, temporal_pool=False):
    import torch
    if temporal_pool:
        from tests._temporal_pool import torch_tsm_tp
        with torch.no_grad():
            return torch_tsm_tp(base_model, shift_place, 12, t, sd=sd)(clips.double()).numpy()
    if non_local:
        from tests._nonlocal import torch_tsm_nl
        with torch.no_grad():
            return torch_tsm_nl(base_model, shift_place, 12, t, sd=sd)(clips.double()).numpy()
    from oracle import tsm_oracle
    sd_t = {k: torch.from_numpy(v) for k, v in sd.items()}
    return tsm_oracle.forward(sd_t, clips, base_model, shift_place, bf16=(dtype == 'bf16'), n_segment=t).numpy()


def run_one(args, base_model, dtype, shift_place='blockres', non_local=False, temporal_pool=False):
    import numpy as np
    import torch
    from workoutdetector_amd.engine import TsmEngine
    from workoutdetector_amd.flops import flops_per_clip
    from workoutdetector_amd.weights import make_state_dict
    b, t, s = args.batch, args.segments, args.size
    sd = make_state_dict(0, 12, base_model=base_model, shift_place=shift_place, non_local=non_local)
    eng = TsmEngine(num_class=12, num_segments=t, height=s, width=s, max_clips=b, state_dict=sd, dtype=dtype,
                    base_model=base_model, shift_place=shift_place, non_local=non_local, temporal_pool=temporal_pool)
    gen = torch.Generator(device='cuda').manual_seed(0)
    clips = torch.randn(b, t, 3, s, s, device='cuda', generator=gen)
    logits = torch.empty(b, 12, device='cuda')
    eng.warmup([b])
    for _ in range(args.warmup):
        eng.forward_device(clips, out=logits)
    torch.cuda.synchronize()
    marks = [torch.cuda.Event(enable_timing=True) for _ in range(args.steps + 1)]
    marks[0].record()
    for i in range(args.steps):
        eng.forward_device(clips, out=logits)
        marks[i + 1].record()
    torch.cuda.synchronize()
    step_ms = sorted(marks[i].elapsed_time(marks[i + 1]) for i in range(args.steps))
    ms = step_ms[len(step_ms) // 2]
    got = logits[:2].cpu().numpy()
    eng.close()
    want = reference_logits(base_model, sd, clips[:2].cpu(), t, dtype, shift_place, non_local, temporal_pool)
    gflop = flops_per_clip(t, s, s, 12, base_model=base_model, non_local=non_local, temporal_pool=temporal_pool) * b / 1e9
    peak = PEAK_F32_MFMA_TFLOPS if dtype == 'f32' else PEAK_BF16_MFMA_TFLOPS
    return {'backbone': base_model, 'dtype': dtype, 'shift_place': shift_place, 'non_local': bool(non_local), 'temporal_pool': bool(temporal_pool), 'batch': b, 'segments': t, 'size': s,
            'ms_per_step': round(ms, 3), 'ms_min': round(step_ms[0], 3), 'ms_max': round(step_ms[-1], 3),
            'clips_per_s': round(b / (ms / 1e3), 1), 'gflop_per_step': round(gflop, 1),
            'tflops': round(gflop / ms, 2), 'peak_tflops': peak, 'peak_frac': round(gflop / ms / peak, 4),
            'logits_err': float(np.abs(got - want).max() / np.abs(want).max()), 'steps': args.steps}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--backbones', default='resnet18,resnet34,resnet50')
    ap.add_argument('--dtypes', default='f32,bf16')
    ap.add_argument('--batch', type=int, default=32)
    ap.add_argument('--segments', type=int, default=8)
    ap.add_argument('--size', type=int, default=224)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--shift-place', default='blockres', help="comma-separated placements: 'blockres', 'block'")
    ap.add_argument('--non-local', action='store_true', help='also run every f32 Bottleneck engine with non_local=True')
    ap.add_argument('--temporal-pool', action='store_true', help='also run every f32 / bf16x3 engine with temporal_pool=True')
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit('backbone_bench.py needs a GPU')
    for dtype in args.dtypes.split(','):
        for base_model in args.backbones.split(','):
            for place in args.shift_place.split(','):
                print(json.dumps(run_one(args, base_model, dtype, place)), flush=True)
                if args.non_local and dtype == 'f32' and base_model in ('resnet50', 'wide_resnet50_2'):
                    print(json.dumps(run_one(args, base_model, dtype, place, non_local=True)), flush=True)
                if args.temporal_pool and dtype in ('f32', 'bf16x3'):
                    print(json.dumps(run_one(args, base_model, dtype, place, temporal_pool=True)), flush=True)


if __name__ == '__main__':
    main()
