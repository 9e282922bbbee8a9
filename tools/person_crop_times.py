"""Launch time of the fused person-crop transform (``tsm_preprocess_clips``: clip windows + crop + resize + normalise + pack
in one launch) beside the unfused centre-crop pair it parallels (``tsm_preprocess`` over every staged frame once, then
``tsm_gather_clips``), for the same 32 clips of 8 frames from 720 x 1280 uint8 frames, into NTHWC4 and NTHWC8B.  DESIGN 4.14.

    python tools/person_crop_times.py <out.json> [clips]

Per layout: 5 warm-up rounds, then 30 rounds in which the fused launch and the unfused pair alternate, each between its own
pair of device events; the median (and min / max) of the 30 is reported.  Bytes of the fused launch = the packed output it
stores + the source pixels inside its boxes (each read at least once; the taps of neighbouring output pixels overlap and
come from cache); GB/s = those bytes over the median."""
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch            # noqa: E402

from workoutdetector_amd import _lib                                                   # noqa: E402
from workoutdetector_amd.engine import gather_clips, preprocess_clips, preprocess_frames   # noqa: E402

out_path = sys.argv[1]
B = int(sys.argv[2]) if len(sys.argv) > 2 else 32
H, W, SIZE, WARM, ROUNDS = 720, 1280, 224, 5, 30
total = 8 * (B - 1) + 16                               # every clip whole: no padded tail in the timed range
g = torch.Generator().manual_seed(0)
even = torch.randint(0, 256, (total // 2 + 1, H, W, 3), dtype=torch.uint8, generator=g).cuda()
even[-1].zero_()                                       # the pad frame the unfused pair stages (the fused launch is not given it)
# person-shaped boxes that drift over the clips, some overhanging the frame
rows = [(40 + 3 * c, 380 + 11 * c - (200 if c % 5 == 0 else 0), 640 + 2 * c, 400 + 7 * (c % 9)) for c in range(B)]
boxes = torch.tensor(rows, dtype=torch.int32).cuda()
inside = sum(max(0, min(t + h, H) - max(t, 0)) * max(0, min(le + w, W) - max(le, 0)) for t, le, h, w in rows) * 8 * 3


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


res = {'clips': B, 'frames': [H, W], 'size': SIZE, 'rounds': ROUNDS, 'device': torch.cuda.get_device_name(0),
       'build': _lib.load().tsm_build_id().decode()}
for name, layout, group_bytes in (('NTHWC4', _lib.LAYOUT_NTHWC4, 16 * SIZE * SIZE), ('NTHWC8B', _lib.LAYOUT_NTHWC8B, 8 * SIZE * SIZE)):
    fused_out = preprocess_clips(even[:-1], boxes, 0, total, 0, B, size=SIZE, layout=layout)
    frames = preprocess_frames(even, layout=layout)
    clips = gather_clips(frames, 0, total, 0, B)

    def fused():
        preprocess_clips(even[:-1], boxes, 0, total, 0, B, size=SIZE, layout=layout, out=fused_out)

    def unfused():
        preprocess_frames(even, layout=layout, out=frames)
        gather_clips(frames, 0, total, 0, B, out=clips)

    for _ in range(WARM):
        fused()
        unfused()
    torch.cuda.synchronize()
    t_f, t_u = [], []
    for _ in range(ROUNDS):
        t_f.append(timed(fused))
        t_u.append(timed(unfused))
    stores = B * 8 * group_bytes
    m = statistics.median(t_f)
    res[name] = {'fused_ms_median': m, 'fused_ms_min': min(t_f), 'fused_ms_max': max(t_f),
                 'unfused_pair_ms_median': statistics.median(t_u), 'unfused_pair_ms_min': min(t_u), 'unfused_pair_ms_max': max(t_u),
                 'fused_store_bytes': stores, 'fused_box_source_bytes': inside, 'fused_gb_per_s': (stores + inside) / (m * 1e-3) / 1e9}
print(json.dumps(res))
with open(out_path, 'w') as f:
    json.dump(res, f, indent=1)
