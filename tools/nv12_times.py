"""What the fused NV12 tap source buys: the NV12 launch of ``tsm_preprocess`` beside what a caller had to do without it, and
the host-to-logits rate of ``video_clip_logits`` from NV12 and from RGB host frames.  DESIGN 4.22.

    python tools/nv12_times.py <out.json>

Launch times, for 264 frames (what 32 clips sample, plus the pad frame) of 1280 x 720 and of 480 x 272, into the f32 packed
layout (NTHWC4, 224 x 224): 3 warm-up rounds, then 10 rounds in which the three forms alternate, each between its own pair of
device events; median (min .. max) of the 10.
  (a) the NV12 launch;
  (b) without it: the same integer formula written in torch ops on the GPU to RGB uint8, then ``tsm_preprocess``;
  (c) ``tsm_preprocess`` alone on RGB that is already there.
(b)'s RGB is checked against ``transform.nv12_to_rgb`` and (a)'s output against (c)'s on that RGB, bit for bit, before timing.

Rates: ``video_clip_logits`` on a seeded synthetic video of 264 frames (33 clips) held in pageable host memory, upload
included, NV12 and RGB alternating, f32 and bf16x3 engines: 2 warm-up rounds (the first one tunes), then 7 timed."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from workoutdetector_amd import _lib, inference_count as ic                                # noqa: E402
from workoutdetector_amd.engine import TsmEngine, preprocess_frames                          # noqa: E402
from workoutdetector_amd.transform import TestTransform, nv12_coefficients, nv12_to_rgb      # noqa: E402
from workoutdetector_amd.weights import make_state_dict                                       # noqa: E402

out_path = sys.argv[1]
N, WARM, ROUNDS = 264, 3, 10
NAME = 'bt601'


def torch_nv12_to_rgb(nv, name=NAME):
    """The conversion a caller writes in torch ops: uint8 [n, 3h/2, w] on the GPU -> uint8 [n, h, w, 3]."""
    y_off, cy, crv, cgu, cgv, cbu = nv12_coefficients(name)
    n, rows, w = nv.shape
    h = rows // 3 * 2
    c = cy * (nv[:, :h].to(torch.int32) - y_off) + 8192
    uv = nv[:, h:].reshape(n, h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    d, e = uv[..., 0], uv[..., 1]
    rgb = torch.stack([(c + crv * e) >> 14, (c + cgu * d + cgv * e) >> 14, (c + cbu * d) >> 14], dim=-1)
    return rgb.clamp_(0, 255).to(torch.uint8)


def synthetic_nv12(seed, n, h, w):
    """uint8 [n, 3h/2, w] on the host: a noisy luma ramp whose level oscillates over time, smooth chroma."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float32)[:, None, None]
    ramp = np.linspace(0, 60, w, dtype=np.float32)[None, None, :]
    out = np.empty((n, 3 * h // 2, w), dtype=np.uint8)
    out[:, :h] = np.clip(100 + 70 * np.sin(2 * np.pi * t / 24) + ramp + rng.integers(0, 24, size=(1, h, w)), 16, 235).astype(np.uint8)
    out[:, h:] = np.clip(128 + 40 * np.cos(2 * np.pi * t / 17) + rng.integers(-8, 8, size=(1, h // 2, w)), 16, 240).astype(np.uint8)
    return torch.from_numpy(out)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {'median': statistics.median(ms), 'min': min(ms), 'max': max(ms)}


res = {'frames': N, 'colorimetry': NAME, 'warmup': WARM, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
       'build': _lib.load().tsm_build_id().decode(), 'launch_ms': {}, 'clips_per_s': {}}
host = {}
for w, h in ((1280, 720), (480, 272)):
    nv_host = synthetic_nv12(w, N, h, w)
    nv = nv_host.cuda()
    rgb = torch_nv12_to_rgb(nv)
    assert np.array_equal(rgb[:2].cpu().numpy(), nv12_to_rgb(nv_host[:2], NAME)) and np.array_equal(rgb[-1].cpu().numpy(), nv12_to_rgb(nv_host[-1], NAME)[0])
    out_a = preprocess_frames(nv, frame_format='nv12', colorimetry=NAME)
    out_c = preprocess_frames(rgb)
    assert torch.equal(out_a.view(torch.int32), out_c.view(torch.int32)), 'the NV12 launch differs from the RGB launch'
    host[(w, h)] = (nv_host, rgb.cpu())

    def form_a():
        preprocess_frames(nv, frame_format='nv12', colorimetry=NAME, out=out_a)

    def form_b():
        preprocess_frames(torch_nv12_to_rgb(nv), out=out_c)

    def form_c():
        preprocess_frames(rgb, out=out_c)

    for _ in range(WARM):
        form_a(), form_b(), form_c()
    torch.cuda.synchronize()
    ta, tb, tc = [], [], []
    for _ in range(ROUNDS):
        ta.append(timed(form_a))
        tb.append(timed(form_b))
        tc.append(timed(form_c))
    res['launch_ms'][f'{w}x{h}'] = {'a_nv12_launch': stats(ta), 'b_torch_convert_then_rgb_launch': stats(tb), 'c_rgb_launch_alone': stats(tc),
                                   'nv12_bytes': int(nv.numel()), 'rgb_bytes': int(rgb.numel()), 'out_bytes': int(out_a.numel()) * 4}
    del nv, rgb, out_a, out_c
    torch.cuda.empty_cache()

tf = TestTransform()
sd = make_state_dict(0, 12)
for dtype in ('f32', 'bf16x3'):
    eng = TsmEngine(num_class=12, num_segments=8, max_clips=32, state_dict=sd, dtype=dtype)
    for (w, h), (nv_host, rgb_host) in host.items():
        n_clips = len(ic.clip_starts(N))

        def run(fmt):
            t0 = time.perf_counter()
            if fmt == 'nv12':
                got = ic.video_clip_logits(eng, nv_host, tf, frame_format='nv12', colorimetry=NAME)
            else:
                got = ic.video_clip_logits(eng, rgb_host, tf)
            return time.perf_counter() - t0, got

        for _ in range(2):
            (_, a), (_, b) = run('nv12'), run('rgb')
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), 'NV12 logits differ from RGB logits'
        t_nv, t_rgb = [], []
        for _ in range(7):
            t_nv.append(run('nv12')[0])
            t_rgb.append(run('rgb')[0])
        res['clips_per_s'][f'{dtype} {w}x{h}'] = {'clips': n_clips,
                                                   'nv12': {k: n_clips / v for k, v in zip(('median', 'max', 'min'), (statistics.median(t_nv), min(t_nv), max(t_nv)))},
                                                   'rgb': {k: n_clips / v for k, v in zip(('median', 'max', 'min'), (statistics.median(t_rgb), min(t_rgb), max(t_rgb)))}}
    eng.close()
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
