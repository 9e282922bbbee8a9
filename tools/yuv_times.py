"""Launch times of ``tsm_preprocess`` from each YUV frame format beside the NV12 and the RGB (uint8) launch.  DESIGN 4.23.

    python tools/yuv_times.py <out.json>

264 frames (what 32 clips sample, plus the pad frame) of 1280 x 720 and of 480 x 272 into the f32 packed layout (NTHWC4,
224 x 224).  All forms run in this one process on the same pictures: one set of planes (a noisy luma ramp, smooth 4:2:0
chroma) arranged as I420, YV12, P010 (random low bytes), NV12, and -- each chroma row written twice -- YUYV and UYVY, so every
form converts to the same RGB frames, which the uint8 launch takes.  Every form's output is checked against the uint8 launch's,
bit for bit, before timing.  3 warm-up rounds, then 10 rounds in which the forms alternate, each between its own pair of device
events; median (min .. max) of the 10.  ``spread`` is (max - min) / median of a form's own 10 rounds: the run-to-run spread a
difference between two forms has to exceed to mean anything."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from workoutdetector_amd import _lib                                                  # noqa: E402
from workoutdetector_amd.engine import preprocess_frames                                # noqa: E402
from workoutdetector_amd.transform import YUV_FORMATS, nv12_coefficients, yuv_to_rgb    # noqa: E402

out_path = sys.argv[1]
N, WARM, ROUNDS = 264, 3, 10
NAME = 'bt601'
FORMS = YUV_FORMATS + ('nv12', 'rgb')


def planes(seed, n, h, w):
    """uint8 Y [n, h, w] and U, V [n, h/2, w/2] on the host: a noisy luma ramp whose level oscillates over time, smooth chroma."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float32)[:, None, None]
    ramp = np.linspace(0, 60, w, dtype=np.float32)[None, None, :]
    y = np.clip(100 + 70 * np.sin(2 * np.pi * t / 24) + ramp + rng.integers(0, 24, size=(1, h, w)), 16, 235).astype(np.uint8)
    u = np.clip(128 + 40 * np.cos(2 * np.pi * t / 17) + rng.integers(-8, 8, size=(1, h // 2, w // 2)), 16, 240).astype(np.uint8)
    v = np.clip(128 - 30 * np.cos(2 * np.pi * t / 13) + rng.integers(-8, 8, size=(1, h // 2, w // 2)), 16, 240).astype(np.uint8)
    return y, u, v


def arrange(fmt, y, u, v, rng):
    """The planes as frames of a format (its uint8 container)."""
    n, h, w = y.shape
    if fmt in ('i420', 'yv12'):
        first, second = (u, v) if fmt == 'i420' else (v, u)
        return np.concatenate([y.reshape(n, -1), first.reshape(n, -1), second.reshape(n, -1)], axis=1).reshape(n, 3 * h // 2, w)
    if fmt in ('nv12', 'p010'):
        nv = np.concatenate([y, np.stack([u, v], axis=-1).reshape(n, h // 2, w)], axis=1)
        if fmt == 'nv12':
            return nv
        return np.stack([rng.integers(0, 256, size=nv.shape, dtype=np.uint8), nv], axis=-1).reshape(n, 3 * h // 2, 2 * w)
    y2, u2, v2 = y.reshape(n, h, w // 2, 2), u.repeat(2, axis=1), v.repeat(2, axis=1)
    group = [y2[..., 0], u2, y2[..., 1], v2] if fmt == 'yuyv' else [u2, y2[..., 0], v2, y2[..., 1]]
    return np.stack(group, axis=-1).reshape(n, h, 2 * w)


def torch_nv12_to_rgb(nv, name=NAME):
    """The integer formula in torch ops on the GPU: uint8 [n, 3h/2, w] -> uint8 [n, h, w, 3] (builds the uint8 launch's input)."""
    y_off, cy, crv, cgu, cgv, cbu = nv12_coefficients(name)
    n, rows, w = nv.shape
    h = rows // 3 * 2
    c = cy * (nv[:, :h].to(torch.int32) - y_off) + 8192
    uv = nv[:, h:].reshape(n, h // 2, w // 2, 2).to(torch.int32) - 128
    uv = uv.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    d, e = uv[..., 0], uv[..., 1]
    rgb = torch.stack([(c + crv * e) >> 14, (c + cgu * d + cgv * e) >> 14, (c + cbu * d) >> 14], dim=-1)
    return rgb.clamp_(0, 255).to(torch.uint8)


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    med = statistics.median(ms)
    return {'median': med, 'min': min(ms), 'max': max(ms), 'spread': (max(ms) - min(ms)) / med}


res = {'frames': N, 'colorimetry': NAME, 'warmup': WARM, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
       'build': _lib.load().tsm_build_id().decode(), 'launch_ms': {}}
for w, h in ((1280, 720), (480, 272)):
    y, u, v = planes(w, N, h, w)
    rng = np.random.default_rng(h)
    src = {}
    for fmt in FORMS[:-1]:
        a = arrange(fmt, y, u, v, rng)
        src[fmt] = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    src['rgb'] = torch_nv12_to_rgb(src['nv12'])
    for fmt in FORMS[:-1]:                  # every arrangement is the same picture, by the host's text
        for j in (0, N - 1):
            assert np.array_equal(yuv_to_rgb(src[fmt][j].cpu().numpy(), fmt, NAME)[0], src['rgb'][j].cpu().numpy()), fmt
    kw = {fmt: ({} if fmt == 'rgb' else dict(frame_format=fmt, colorimetry=NAME)) for fmt in FORMS}
    out = {fmt: preprocess_frames(src[fmt], **kw[fmt]) for fmt in FORMS}
    for fmt in FORMS:
        assert torch.equal(out[fmt].view(torch.int32), out['rgb'].view(torch.int32)), f'the {fmt} launch differs from the RGB launch'

    def form(fmt):
        preprocess_frames(src[fmt], out=out[fmt], **kw[fmt])

    for _ in range(WARM):
        for fmt in FORMS:
            form(fmt)
    torch.cuda.synchronize()
    ms = {fmt: [] for fmt in FORMS}
    for _ in range(ROUNDS):
        for fmt in FORMS:
            ms[fmt].append(timed(lambda: form(fmt)))
    res['launch_ms'][f'{w}x{h}'] = {fmt: dict(stats(ms[fmt]), bytes=int(src[fmt].numel())) for fmt in FORMS}
    res['launch_ms'][f'{w}x{h}']['out_bytes'] = int(out['rgb'].numel()) * 4
    del src, out
    torch.cuda.empty_cache()
print(json.dumps(res))
os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
