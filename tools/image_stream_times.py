"""Times of the image model on streams (``tsm_preprocess_windows`` in image mode, ``ImageStreamBatcher``) on one GPU, all in
one process:

* the transform alone into NTHWC4, 32 frames of one resolution and 32 frames over four (8 each, interleaved in batch order,
  and grouped by resolution): (a) the one launch of ``preprocess_image_windows``; (b) what the library could do before it:
  one ``tsm_preprocess_image`` launch per resolution -- into its slice of the batch where the slices are contiguous, else
  into a buffer of its own plus an ``index_copy_`` scatter.  (a) and (b) alternate round by round; device events.
* ``ImageStreamBatcher.step()`` end to end on the ResNet-18 image model -- upload, transform, forward, arg-max, the 4 bytes
  per frame back; a host clock around the call, which ends in its synchronising copy -- for 1 stream and for 32 streams (one
  frame each, the four resolutions in turn), RGB and NV12; the ``push`` calls of a round are timed apart.

Medians and min .. max of ROUNDS rounds after WARM warm-up rounds.

    python tools/image_stream_times.py out.json
"""
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np      # noqa: E402
import torch            # noqa: E402

from workoutdetector_amd import _lib                                                                        # noqa: E402
from workoutdetector_amd.engine import create_image_model, preprocess_image, preprocess_image_windows       # noqa: E402
from workoutdetector_amd.streaming import ImageStreamBatcher                                                # noqa: E402
from workoutdetector_amd.transform import image_window_arena, rgb_to_nv12                                   # noqa: E402

out_path = sys.argv[1]
SIZES = {'1280x720': (720, 1280), '854x480': (480, 854), '640x360': (360, 640), '480x272': (272, 480)}      # name: (h, w)
N, RESIZE, CROP, WARM, ROUNDS = 32, 256, 224, 5, 30
LAYOUT = _lib.LAYOUT_NTHWC4
rng = np.random.default_rng(0)
assert torch.cuda.is_available(), 'this tool measures on a GPU'


def stats(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms)}


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternate(fns):
    """{name: [ms per round]} of the given calls, alternating within every round."""
    for _ in range(WARM):
        for fn in fns.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in fns}
    for _ in range(ROUNDS):
        for k, fn in fns.items():
            ms[k].append(event_ms(fn))
    return ms


def transform_case(shapes):
    """The frames of one batch (shapes in batch order): the one-launch route and the per-resolution route."""
    frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
    desc, offsets, tables, nbytes = image_window_arena(shapes, 1, RESIZE, CROP)
    arena = np.zeros(nbytes, dtype=np.uint8)
    for f, off in zip(frames, offsets):
        arena[off:off + f.size] = f.reshape(-1)
    for off, block in tables:
        arena[off:off + block.nbytes] = block.view(np.uint8)
    arena_d, desc_d = torch.from_numpy(arena).cuda(), torch.from_numpy(desc).cuda()
    out_a = torch.empty((N, 1, CROP, CROP, 4), dtype=torch.float32, device='cuda')
    out_b = torch.empty((N, CROP, CROP, 4), dtype=torch.float32, device='cuda')
    groups = {}
    for i, s in enumerate(shapes):
        groups.setdefault(s, []).append(i)
    staged = {s: torch.from_numpy(np.stack([frames[i] for i in idx])).cuda() for s, idx in groups.items()}
    contiguous = all(idx == list(range(idx[0], idx[0] + len(idx))) for idx in groups.values())
    index = {s: torch.tensor(idx, device='cuda') for s, idx in groups.items()}
    tmp = {s: torch.empty((len(idx), CROP, CROP, 4), dtype=torch.float32, device='cuda') for s, idx in groups.items()}

    def one_launch():
        preprocess_image_windows(arena_d, desc_d, N, 1, resize=RESIZE, crop=CROP, out_layout=LAYOUT, out=out_a)

    def per_resolution():
        for s, idx in groups.items():
            if contiguous:
                preprocess_image(staged[s], RESIZE, CROP, out_layout=LAYOUT, out=out_b[idx[0]:idx[0] + len(idx)])
            else:
                preprocess_image(staged[s], RESIZE, CROP, out_layout=LAYOUT, out=tmp[s])
                out_b.index_copy_(0, index[s], tmp[s])
    ms = alternate({'one_launch': one_launch, 'per_resolution': per_resolution})
    assert torch.equal(out_a.view(torch.int32).view(out_b.shape), out_b.view(torch.int32)), 'the two routes differ'
    a, b = stats(ms['one_launch']), stats(ms['per_resolution'])
    return {'resolutions': len(groups), 'launches_per_resolution_route': len(groups), 'scatter': not contiguous,
            'preprocess_image_windows': a, 'preprocess_image_per_resolution': b, 'ratio': a['median_ms'] / b['median_ms']}


def step_case(eng, n_streams, fmt):
    shapes = [list(SIZES.values())[i % 4] for i in range(n_streams)]
    sb = ImageStreamBatcher(eng, frame_format=fmt)
    push_ms, step_ms = [], []
    for r in range(WARM + ROUNDS):
        frames = [rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8) for h, w in shapes]
        if fmt == 'nv12':
            frames = [rgb_to_nv12(f)[0] for f in frames]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i, f in enumerate(frames):
            sb.push(i, f)
        t1 = time.perf_counter()
        got = sb.step()                              # (ends in the synchronising copy of the arg-maxes)
        t2 = time.perf_counter()
        assert sum(len(v) for v in got.values()) == n_streams
        if r >= WARM:
            push_ms.append((t1 - t0) * 1e3)
            step_ms.append((t2 - t1) * 1e3)
    for i in range(n_streams):
        sb.close(i)
    return {'streams': n_streams, 'frames_per_step': n_streams, 'frame_format': fmt, 'step': stats(step_ms), 'push_all_streams': stats(push_ms)}


res = {'what': 'the image model on streams: tsm_preprocess_windows in image mode against one tsm_preprocess_image launch per resolution, '
               'and ImageStreamBatcher.step() end to end; one MI355X',
       'device': torch.cuda.get_device_name(0), 'build': _lib.load().tsm_build_id().decode(), 'frames': N, 'resize': RESIZE, 'crop': CROP,
       'layout': 'NTHWC4', 'warm': WARM, 'rounds': ROUNDS, 'sizes_w_x_h': list(SIZES), 'transform': {}, 'step': []}
four = list(SIZES.values())
res['transform']['one_resolution_1280x720'] = transform_case([SIZES['1280x720']] * N)
res['transform']['four_resolutions_interleaved'] = transform_case([four[i % 4] for i in range(N)])
res['transform']['four_resolutions_grouped'] = transform_case([four[i // 8] for i in range(N)])

eng = create_image_model(num_class=2, base_model='resnet18', max_frames=32, resize=RESIZE, crop=CROP)
eng.warmup([1, 32])
x = torch.empty((32, 1, CROP, CROP, 4), dtype=torch.float32, device='cuda').normal_()
x[..., 3] = 0
fwd = []
for _ in range(WARM + ROUNDS):
    eng.forward_device(x, layout=eng.packed_layout)
    fwd.append(eng.last_forward_ms)
res['forward_32_frames'] = dict(stats(fwd[WARM:]), model='resnet18 f32')
for n_streams in (1, 32):
    for fmt in ('rgb', 'nv12'):
        res['step'].append(step_case(eng, n_streams, fmt))
eng.close()
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
