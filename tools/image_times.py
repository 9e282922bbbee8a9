"""Launch time of the image model's transform (``tsm_preprocess_image``: Pillow's antialiased 8-bit resample + crop + normalise
+ pack in one launch) beside the existing ``tsm_preprocess`` on the same frames (ATen's bilinear without antialias: the cost
floor of a four-tap gather), for 32 frames of 720 x 1280 uint8 into NTHWC4 and NTHWC8B; then the frame rate of
``count_by_image_model`` on an R18 f32 image engine with ``max_frames=32``.  DESIGN 4.15.

    python tools/image_times.py <out.json> [frames]

Per layout: 5 warm-up rounds, then 30 rounds in which the two launches alternate, each between its own pair of device events;
the median (and min / max) of the 30 is reported.  ``support_bytes`` = the source pixels under the crop window's support (every
one is read at least once; the taps of neighbouring outputs overlap and come from cache), ``store_bytes`` the packed output;
``hbm_floor_ms`` = their sum at HBM_GBPS (the nominal peak, stated in the file).  End to end: 8 batches of 32 host frames
through staging, transform, forward and vote, 3 timed passes after one warm-up, wall clock around a final synchronise."""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch            # noqa: E402

from workoutdetector_amd import _lib                                                   # noqa: E402
from workoutdetector_amd import inference_count as ic                                  # noqa: E402
from workoutdetector_amd.engine import create_image_model, preprocess_frames, preprocess_image   # noqa: E402
from workoutdetector_amd.transform import crop_offsets, pil_resample_tables, resized_hw          # noqa: E402

out_path = sys.argv[1]
N = int(sys.argv[2]) if len(sys.argv) > 2 else 32
H, W, RESIZE, CROP, WARM, ROUNDS, HBM_GBPS = 720, 1280, 256, 224, 5, 30, 8000.0
g = torch.Generator().manual_seed(0)
host = torch.randint(0, 256, (N, H, W, 3), dtype=torch.uint8, generator=g)
frames = host.cuda()

nh, nw = resized_hw(H, W, RESIZE)
top, left = crop_offsets(nh, nw, CROP)
span = []
for size, new, first in ((W, nw, left), (H, nh, top)):
    b = pil_resample_tables(size, new)[0]
    span.append(int(b[first + CROP - 1].sum()) - int(b[first, 0]))
support = N * span[0] * span[1] * 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


res = {'frames': N, 'frame_hw': [H, W], 'resize': RESIZE, 'crop': CROP, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
       'build': _lib.load().tsm_build_id().decode(), 'support_window_hw': [span[1], span[0]], 'support_bytes': support,
       'hbm_gb_per_s_assumed': HBM_GBPS}
for name, layout, px_bytes in (('NTHWC4', _lib.LAYOUT_NTHWC4, 16), ('NTHWC8B', _lib.LAYOUT_NTHWC8B, 8)):
    new_out = preprocess_image(frames, RESIZE, CROP, out_layout=layout)
    old_out = preprocess_frames(frames, RESIZE, CROP, scale_255=True, layout=layout)

    def new():
        preprocess_image(frames, RESIZE, CROP, out_layout=layout, out=new_out)

    def old():
        preprocess_frames(frames, RESIZE, CROP, scale_255=True, layout=layout, out=old_out)

    for _ in range(WARM):
        new()
        old()
    torch.cuda.synchronize()
    t_n, t_o = [], []
    for _ in range(ROUNDS):
        t_n.append(timed(new))
        t_o.append(timed(old))
    stores = N * CROP * CROP * px_bytes
    m = statistics.median(t_n)
    res[name] = {'preprocess_image_ms_median': m, 'preprocess_image_ms_min': min(t_n), 'preprocess_image_ms_max': max(t_n),
                 'tsm_preprocess_ms_median': statistics.median(t_o), 'tsm_preprocess_ms_min': min(t_o),
                 'tsm_preprocess_ms_max': max(t_o), 'ratio_to_tsm_preprocess': m / statistics.median(t_o),
                 'store_bytes': stores, 'hbm_floor_ms': (support + stores) / (HBM_GBPS * 1e9) * 1e3,
                 'gb_per_s': (support + stores) / (m * 1e-3) / 1e9}

# ---- end to end: R18 f32, max_frames = 32 ----
eng = create_image_model(num_class=2, max_frames=32, resize=RESIZE, crop=CROP)
eng.warmup([min(N, 32)])
video = host.repeat(8, 1, 1, 1) if N * 8 * H * W * 3 <= (1 << 31) else host
ic.count_by_image_model(eng, video)
torch.cuda.synchronize()
walls = []
for _ in range(3):
    t0 = time.perf_counter()
    ic.count_by_image_model(eng, video)
    torch.cuda.synchronize()
    walls.append(time.perf_counter() - t0)
x = preprocess_image(frames[:32], RESIZE, CROP, out_layout=eng.packed_layout)
fwd = []
for _ in range(10):
    eng.forward_device(x.view((x.shape[0], 1) + tuple(x.shape[1:])), layout=eng.packed_layout)
    fwd.append(eng.last_forward_ms)
fwd_ms = statistics.median(fwd[2:])
res['end_to_end'] = {'model': 'resnet18 f32', 'max_frames': 32, 'video_frames': int(video.shape[0]),
                     'wall_s_median': statistics.median(walls), 'wall_s_min': min(walls), 'wall_s_max': max(walls),
                     'frames_per_s': int(video.shape[0]) / statistics.median(walls),
                     'forward_ms_32_frames': fwd_ms,
                     'preprocess_share_of_forward': res['NTHWC4']['preprocess_image_ms_median'] * min(32, N) / N / fwd_ms}
eng.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
